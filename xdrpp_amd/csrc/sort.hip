// Sorting a record batch on gfx950: the launchers of sort_kernels.h.
//
//   xdrg_sort_workspace_size  bytes xdrg_sort needs for n records
//   xdrg_sort                 std::stable_sort by xdr::operator< (xdrpp/
//                             types.h:946-1062) as a permutation, the groups
//                             of equivalent records marked (std::unique)
//
// xdrg_sort validates its arguments on the host before the first HIP call
// and launches kernels only (no memset or memcpy nodes, no sync: xdrgpu.h
// "Graph capture"); the plan's first compare or sort on a device uploads the
// class table (cmp_upload).  The launches depend on n alone: the number of
// sortable records stays on the device (sort_kernels.h).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "compare_host.h"
#include "sort_kernels.h"

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

namespace {

constexpr uint64_t kSortMaxN = 1ull << 31;

// Workspace: two permutation buffers, the flag bytes, the tile counts.
size_t ws_perm(uint64_t n) { return align256(n * 4u); }
size_t ws_flags(uint64_t n) { return align256(n); }

// The passes of width 1 .. 128 run in one launch, a tile's entries in LDS
// (k_sort_tile), or as passes in global memory like the wider ones with
// XDRG_SORT_TILE=0 in the environment (tools/gpu/time_sort.py measures
// both).
bool tile_pass() {
  const char *v = std::getenv("XDRG_SORT_TILE");
  return !(v && v[0] == '0' && !v[1]);
}

template <bool LDSOPS>
void launch(const sort_batch &B, uint32_t nb, size_t lds, uint32_t *perm, uint8_t *first, uint64_t *counts,
            uint32_t *w0, uint32_t *w1, uint8_t *flags, unsigned long long *tiles, hipStream_t s) {
  const uint32_t n = B.n;
  const bool tile = tile_pass();
  // passes: widths w0 .. < n, the first one from `start`
  const uint32_t start = tile ? kTileThreads : 1u;
  uint32_t passes = tile ? 1u : 0u;
  for (uint64_t w = start; w < n; w <<= 1) ++passes;
  if (n < 2u) passes = 0u;
  uint32_t *cur = passes ? w0 : perm, *other = w1;
  k_sort_classify<LDSOPS><<<nb, kTileThreads, lds, s>>>(B, flags, tiles);
  k_tile_scan<1, 1><<<1, kScanThreads, 0, s>>>(tiles, static_cast<unsigned long long *>(nullptr), uint64_t(nb),
                                               count_total{counts});
  k_sort_emit<><<<nb, kTileThreads, 0, s>>>(n, flags, tiles, counts, cur);
  uint32_t left = passes;
  auto dst = [&]() { return --left ? other : perm; };  // the last pass lands in perm
  if (passes && tile) {
    uint32_t *o = dst();
    k_sort_tile<LDSOPS><<<nb, kTileThreads, lds, s>>>(B, counts, cur, o);
    other = cur;
    cur = o;
  }
  for (uint64_t w = start; w < n && left; w <<= 1) {
    uint32_t *o = dst();
    k_sort_merge<LDSOPS><<<nb, kTileThreads, lds, s>>>(B, counts, uint32_t(w), cur, o);
    other = cur;
    cur = o;
  }
  k_sort_first<LDSOPS><<<nb, kTileThreads, lds, s>>>(B, counts, perm, first, tiles);
  k_tile_scan<1, 1><<<1, kScanThreads, 0, s>>>(tiles, static_cast<unsigned long long *>(nullptr), uint64_t(nb),
                                               sort_distinct{counts});
}

}  // namespace

extern "C" {

size_t xdrg_sort_workspace_size(const xdrg_plan *plan, uint64_t n) {
  (void)plan;  // (every plan sorts by the walk; a key path for fixed plans would size by the plan)
  if (n > kSortMaxN) return 0;
  return 2 * ws_perm(n) + ws_flags(n) + ws_tiles(n);
}

int xdrg_sort(const xdrg_plan *plan, const void *d_recs, const void *d_heap, uint64_t heap_len, uint64_t n,
              uint32_t *d_perm, uint8_t *d_first, uint64_t *d_counts, void *d_workspace, size_t workspace_bytes,
              void *stream) {
  if (!plan || (n && (!d_recs || !d_perm || !d_counts || !d_workspace))) return XDRG_EINVAL;
  if (!d_heap && heap_len) return XDRG_EINVAL;
  if (n > kSortMaxN) return XDRG_EUNSUPPORTED;
  if (n && workspace_bytes < xdrg_sort_workspace_size(plan, n)) return XDRG_EINVAL;
  const bool var = plan->path == XDRG_PATH_VAR;
  if (misaligned(d_recs, var ? 7 : 3) || misaligned(d_heap, 3) || misaligned(d_workspace, 15) ||
      misaligned(d_perm, 3) || misaligned(d_counts, 7))
    return XDRG_EALIGN;
  int rc = cmp_classes_ready(plan);
  if (rc != XDRG_OK) return rc;
  if (n == 0) return XDRG_OK;
  const dev_tables *T = nullptr;
  rc = plan_tables(plan, &T);
  if (rc != XDRG_OK) return rc;
  cmp_tables C = {};
  rc = cmp_upload(plan, &C);
  if (rc != XDRG_OK) return rc;
  const uint32_t nops = uint32_t(plan->ops.size());
  const sort_batch B = {static_cast<const uint8_t *>(d_recs), static_cast<const uint8_t *>(d_heap), heap_len,
                        uint32_t(n), plan->stride, T->d_ops, C.d_info, nops, T->d_table};
  uint8_t *ws = static_cast<uint8_t *>(d_workspace);
  uint32_t *w0 = reinterpret_cast<uint32_t *>(ws), *w1 = reinterpret_cast<uint32_t *>(ws + ws_perm(n));
  uint8_t *flags = ws + 2 * ws_perm(n);
  unsigned long long *tiles = reinterpret_cast<unsigned long long *>(flags + ws_flags(n));
  const uint32_t nb = uint32_t(tiles_of(n));
  const size_t lds = size_t(nops) * (sizeof(xdrg_op) + 4u);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (lds <= kCmpLdsOps)
    launch<true>(B, nb, lds, d_perm, d_first, d_counts, w0, w1, flags, tiles, s);
  else
    launch<false>(B, nb, 0, d_perm, d_first, d_counts, w0, w1, flags, tiles, s);
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

}  // extern "C"
