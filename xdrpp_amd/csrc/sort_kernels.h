// std::stable_sort / std::unique of a record batch by xdr::operator< on
// gfx950 (xdrg_sort): a permutation, not moved records.  The comparator is
// the pair walk of compare_kernels.h (cmp_walk_pair), for every plan.
//
//   k_sort_classify  a lane per record: rec <=> rec.  EQUAL makes the record
//                    sortable (a NaN the walk reaches, a reference outside
//                    the heap or nesting past the register frames do not);
//                    one flag byte a record, one count a tile.
//   (k_tile_scan)    the tile counts to offsets, their total m to counts[0].
//   k_sort_emit      the sortable indices, in input order, to perm[0..m), the
//                    others behind them, in input order.
//   k_sort_tile      the merge passes of width 1..128 of a tile's 256
//                    entries, in LDS between barriers.
//   k_sort_merge     one merge pass of width w by rank: lane k < m owns
//                    x = in[k], finds its run and the sibling run, counts by
//                    binary search the sibling's elements that go before x
//                    (ties: the left run's element first, which is the key
//                    (record, index), as a run's indices ascend and the left
//                    run's are all lower) and writes x to the pair's base +
//                    its own rank + that count.  No lane waits for another.
//   k_sort_first     first[k] = k == 0 || rec[perm[k-1]] < rec[perm[k]] for
//                    k < m, 1 behind; the ones below m counted per tile.
//
// m is read from counts[0] by the kernels, never by the host: every launch
// is sized by n, and lanes at or past m copy their entry.  Nothing a
// comparator returns can take a store out of bounds: a destination is the
// pair's base plus two ranks that the run lengths bound, entries are only
// ever copied, and an entry that is no index (which a comparator that is no
// order could leave behind, through a position two lanes both chose) is
// carried along and never used to address a record.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_kernels.h"
#include "compare_kernels.h"

namespace xdrg {
namespace dev {

// What every lane needs to compare two records of the batch.
struct sort_batch {
  const uint8_t *recs, *heap;
  uint64_t heap_len;
  uint32_t n, stride;  // (n <= 2^31)
  const xdrg_op *g_ops;
  const uint32_t *g_info;
  uint32_t nops;
  const uint32_t *table;
};

template <bool LDSOPS>
struct sort_walk {
  const sort_batch &B;
  const xdrg_op *ops;
  const uint32_t *info;
  // every lane of the workgroup constructs it (LDSOPS: loads, then a barrier)
  __device__ __forceinline__ explicit sort_walk(const sort_batch &b) : B(b), ops(b.g_ops), info(b.g_info) {
    if constexpr (LDSOPS) cmp_lds_ops(b.g_ops, b.g_info, b.nops, &ops, &info);
  }
  __device__ __forceinline__ int8_t operator()(uint32_t a, uint32_t b) const {
    return cmp_walk_pair<LDSOPS>(B.recs + static_cast<uint64_t>(a) * B.stride,
                                 B.recs + static_cast<uint64_t>(b) * B.stride, B.heap, B.heap_len, B.heap,
                                 B.heap_len, ops, info, B.table);
  }
};

__device__ __forceinline__ uint32_t sort_m(const uint64_t *counts, uint32_t n) {
  const uint64_t m = counts[0];
  return m < n ? static_cast<uint32_t>(m) : n;
}

template <bool LDSOPS>
__global__ __launch_bounds__(256) void k_sort_classify(const sort_batch B, uint8_t *__restrict__ flags,
                                                       unsigned long long *__restrict__ tile_cnt) {
  const sort_walk<LDSOPS> walk(B);
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  bool ok = false;
  if (i < B.n) {
    ok = walk(static_cast<uint32_t>(i), static_cast<uint32_t>(i)) == XDRG_CMP_EQUAL;
    flags[i] = ok;
  }
  tile_reduce(0ull, ok, nullptr, tile_cnt);
}

// tile_cnt: scanned (the sortable records before the tile).
template <class = void>
__global__ __launch_bounds__(256) void k_sort_emit(uint32_t n, const uint8_t *__restrict__ flags,
                                                   const unsigned long long *__restrict__ tile_cnt,
                                                   const uint64_t *__restrict__ counts, uint32_t *__restrict__ perm) {
  __shared__ uint32_t wc[kTileThreads / 64];
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const bool ok = i < n && flags[i];
  const unsigned long long bal = __ballot(ok);
  if (lane == 0u) wc[wid] = __popcll(bal);
  __syncthreads();
  uint64_t before = tile_cnt[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));  // sortable ones before i
  for (uint32_t k = 0; k < wid; ++k) before += wc[k];
  if (i >= n) return;
  const uint64_t pos = ok ? before : sort_m(counts, n) + (i - before);
  if (pos < n) perm[pos] = static_cast<uint32_t>(i);
}

// Where x = entry k (k < m) goes in the merge of its run of width w with the
// sibling run; get(j) = entry j of the pass's input, j in [k's pair) only.
template <class WALK, class GET>
__device__ __forceinline__ uint32_t sort_rank(const WALK &walk, GET &&get, uint32_t k, uint32_t x, uint32_t w,
                                              uint32_t m, uint32_t n) {
  const uint32_t base = k & ~(2u * w - 1u);  // (w is a power of two; base + 2 w <= 2^31)
  const uint32_t mid = min(base + w, m), end = min(base + 2u * w, m);
  const bool left = k < mid;
  const uint32_t s0 = left ? mid : base;
  uint32_t lo = s0, hi = left ? end : mid;
  if (x >= n) return k;  // no index: stays where it is
  while (lo < hi) {
    const uint32_t j = (lo + hi) >> 1;
    const uint32_t y = get(j);
    // y goes before x: from the right run when y < x, from the left run
    // unless x < y.  Anything but LESS (which sortable records never give
    // besides EQUAL and GREATER) is "not less".
    const bool less = y < n && walk(left ? y : x, left ? x : y) == XDRG_CMP_LESS;
    if (left ? less : !less) lo = j + 1u; else hi = j;
  }
  return base + (k - (left ? base : mid)) + (lo - s0);
}

template <bool LDSOPS>
__global__ __launch_bounds__(256) void k_sort_merge(const sort_batch B, const uint64_t *__restrict__ counts,
                                                    uint32_t w, const uint32_t *__restrict__ in,
                                                    uint32_t *__restrict__ out) {
  const sort_walk<LDSOPS> walk(B);
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  if (i >= B.n) return;
  const uint32_t k = static_cast<uint32_t>(i), m = sort_m(counts, B.n);
  const uint32_t x = in[k];
  const uint32_t at = k < m ? sort_rank(walk, [&](uint32_t j) { return in[j]; }, k, x, w, m, B.n) : k;
  out[at] = x;  // (at < min(base + 2 w, m) <= n, or k)
}

// The passes of width 1 .. kTileThreads / 2 of one tile.
template <bool LDSOPS>
__global__ __launch_bounds__(256) void k_sort_tile(const sort_batch B, const uint64_t *__restrict__ counts,
                                                   const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
  __shared__ uint32_t ent[kTileThreads];
  const sort_walk<LDSOPS> walk(B);
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kTileThreads, i = t0 + threadIdx.x;
  const uint32_t m = sort_m(counts, B.n);
  const uint32_t mt = m > t0 ? static_cast<uint32_t>(min(static_cast<uint64_t>(kTileThreads), m - t0)) : 0u;
  const uint32_t k = threadIdx.x;
  uint32_t x = i < B.n ? in[i] : 0u;
  ent[k] = x;
  __syncthreads();
  for (uint32_t w = 1; w < kTileThreads; w <<= 1) {  // (uniform: every lane takes the barriers)
    const uint32_t at = k < mt ? sort_rank(walk, [&](uint32_t j) { return ent[j]; }, k, x, w, mt, B.n) : k;
    __syncthreads();  // every search of this pass is done
    ent[at] = x;      // (at < kTileThreads)
    __syncthreads();
    x = ent[k];  // the lane owns position k of the next pass, not the entry it moved
  }
  if (i < B.n) out[i] = x;
}

template <bool LDSOPS>
__global__ __launch_bounds__(256) void k_sort_first(const sort_batch B, const uint64_t *__restrict__ counts,
                                                    const uint32_t *__restrict__ perm, uint8_t *__restrict__ first,
                                                    unsigned long long *__restrict__ tile_cnt) {
  const sort_walk<LDSOPS> walk(B);
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint32_t m = sort_m(counts, B.n);
  bool one = false;
  if (i < m) {
    one = i == 0u;
    if (!one) {
      const uint32_t p = perm[i - 1u], q = perm[i];
      one = p < B.n && q < B.n && walk(p, q) == XDRG_CMP_LESS;
    }
  }
  if (first && i < B.n) first[i] = i < m ? one : 1u;
  tile_reduce(0ull, one, nullptr, tile_cnt);
}

// counts[1] = the distinct values.
struct sort_distinct {
  uint64_t *counts;
  __device__ void operator()(const unsigned long long (&t)[1], uint32_t lane) const {
    if (lane == 0) counts[1] = t[0];
  }
};

}  // namespace dev
}  // namespace xdrg
