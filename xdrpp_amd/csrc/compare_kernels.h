// xdr::operator== / operator<=> of record batches on gfx950 (xdrg_compare):
// the comparison operators of xdrpp/types.h:946-1062 (XDRPP_STRONG_ORDER =
// 0) and pointer's at :647-657, over native records.
//
//   k_cmp_fixed   fixed plans whose native stride is a multiple of 16: a
//                 lane owns one 16-byte chunk position of the record and
//                 keeps its four words' program (cmp_word, plan.h) in
//                 registers, as k_fixed_reg keeps its selectors.  It loads
//                 the chunk of a and of b (coalesced 16-byte loads),
//                 evaluates its words and produces a key: (first word that
//                 is not equivalent) << 2 | result, all ones when all four
//                 are.  The record's result is the key of the lowest word
//                 index, a segmented minimum over the stride / 16 lanes of
//                 the record by cross-lane reads (no LDS, no atomics).  A
//                 wave holds whole records only (64 / cpr of them a step),
//                 so a segment never leaves its wave; records of more than
//                 64 chunks take a wave each, in steps.  Identical bytes
//                 are not "equal" (a NaN is unordered) and differing bytes
//                 not "different" (-0.0, bool 2 against bool 1), so float
//                 and bool words are always evaluated.
//   k_cmp_walk    everything else: one lane walks one pair with a single
//                 pc, both records following the same ops until the first
//                 difference.  Element subroutines use the register frame
//                 stack of sub_kernels.h (reg_stack_t: shifted frames,
//                 every index a constant, no private memory -- see there
//                 why frames must not live in scratch), each frame with a
//                 second cursor for b.  A container in tail position takes
//                 over the top frame (sub_tail), so a linked list compares
//                 in one frame at any length; a pair that would need more
//                 than XDRG_SUB_FRAMES open frames is XDRG_CMP_DEEP.
//
// Results inside the kernels: R_LESS, R_GREATER, R_UNORD, R_EQ (ordered so
// that the key of an all-equal chunk is the largest).
#pragma once
#include <hip/hip_runtime.h>

#include "plan.h"
#include "sub_kernels.h"

namespace xdrg {
namespace dev {

enum : uint32_t { R_LESS = 0, R_GREATER = 1, R_UNORD = 2, R_EQ = 3 };
constexpr uint32_t kCmpAllEq = 0xffffffffu;

__device__ __forceinline__ int8_t cmp_result(uint32_t r) {
  return r == R_LESS ? XDRG_CMP_LESS : r == R_GREATER ? XDRG_CMP_GREATER : r == R_UNORD ? XDRG_CMP_UNORDERED
                                                                                        : XDRG_CMP_EQUAL;
}
template <class T> __device__ __forceinline__ uint32_t cmp_ord(T a, T b) {
  return a < b ? R_LESS : a > b ? R_GREATER : R_EQ;
}
// IEEE: -0.0 == +0.0; a NaN is unordered against everything, itself included
template <class T> __device__ __forceinline__ uint32_t cmp_ieee(T a, T b) {
  return a < b ? R_LESS : a > b ? R_GREATER : a == b ? R_EQ : R_UNORD;
}
__device__ __forceinline__ uint32_t cmp_w32(uint32_t cls, uint32_t a, uint32_t b) {
  if (cls == XDRG_CLASS_SIGNED) return cmp_ord(static_cast<int32_t>(a), static_cast<int32_t>(b));
  if (cls == XDRG_CLASS_IEEE) return cmp_ieee(__uint_as_float(a), __uint_as_float(b));
  if (cls == XDRG_CLASS_BOOL) return cmp_ord(a != 0u, b != 0u);
  return cmp_ord(a, b);
}
__device__ __forceinline__ uint32_t cmp_w64(uint32_t cls, uint64_t a, uint64_t b) {
  if (cls == XDRG_CLASS_SIGNED) return cmp_ord(static_cast<int64_t>(a), static_cast<int64_t>(b));
  if (cls == XDRG_CLASS_IEEE) return cmp_ieee(__longlong_as_double(a), __longlong_as_double(b));
  return cmp_ord(a, b);
}
// bytes in memory order as unsigned chars: the first differing byte decides
__device__ __forceinline__ uint32_t cmp_mem32(uint32_t a, uint32_t b) { return cmp_ord(bswap32(a), bswap32(b)); }

// ------------------------------------------------------- fixed: chunk lanes
// 0x01 in every byte of m whose byte of v is nonzero (bool: any nonzero
// native byte is true)
__device__ __forceinline__ uint32_t bool_bytes(uint32_t v, uint32_t m) {
  const uint32_t t = v & m;
  return ((((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u) >> 7;
}
__device__ __forceinline__ uint32_t cmp_word_eval(const cmp_word &w, uint32_t a0, uint32_t a1, uint32_t b0,
                                                  uint32_t b1) {
  switch (w.kind) {
  case CW_U32: return cmp_ord(a0, b0);
  case CW_S32: return cmp_ord(static_cast<int32_t>(a0), static_cast<int32_t>(b0));
  case CW_F32: return cmp_ieee(__uint_as_float(a0), __uint_as_float(b0));
  case CW_BYTES: return cmp_mem32((a0 & w.bytes) | bool_bytes(a0, w.bools), (b0 & w.bytes) | bool_bytes(b0, w.bools));
  case CW_U64: return cmp_w64(XDRG_CLASS_UNSIGNED, a0 | (uint64_t(a1) << 32), b0 | (uint64_t(b1) << 32));
  case CW_S64: return cmp_w64(XDRG_CLASS_SIGNED, a0 | (uint64_t(a1) << 32), b0 | (uint64_t(b1) << 32));
  case CW_F64: return cmp_w64(XDRG_CLASS_IEEE, a0 | (uint64_t(a1) << 32), b0 | (uint64_t(b1) << 32));
  default: return R_EQ;  // CW_PAD
  }
}
// The key of one chunk: its first word (record word index w0 + i) that is
// not equivalent, or kCmpAllEq.
__device__ __forceinline__ uint32_t cmp_chunk_key(const cmp_word (&w)[4], const u32x4 &a, const u32x4 &b,
                                                  uint32_t w0) {
  const uint32_t av[5] = {a.x, a.y, a.z, a.w, 0u}, bv[5] = {b.x, b.y, b.z, b.w, 0u};
  uint32_t key = kCmpAllEq;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    const uint32_t r = cmp_word_eval(w[i], av[i], av[i + 1], bv[i], bv[i + 1]);
    if (r != R_EQ) key = ((w0 + i) << 2) | r;
  }
  return key;
}

// cpr = 16-byte chunks per record.  LONG = false (cpr <= 64): a wave step
// compares 64 / cpr whole records; LONG: a record per wave, 64 chunks a step.
template <bool LONG>
__global__ __launch_bounds__(256) void k_cmp_fixed(const u32x4 *__restrict__ a, const u32x4 *__restrict__ b,
                                                   uint64_t n, uint32_t cpr, const cmp_word *__restrict__ prog,
                                                   int8_t *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> 6;
  if constexpr (!LONG) {
    const uint32_t R = 64u / cpr;  // records a wave step holds
    const uint32_t q = lane % cpr, rl = lane / cpr;
    cmp_word w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = prog[4u * q + i];
    // One step per wave over a one-shot grid (the launcher's): four steps a
    // turn with their eight loads issued first measured slower, 0.106 against
    // 0.089 ms for 1M rec128 pairs (profiles/compare/time_compare_unroll4.txt).
    for (uint64_t g = wave; g * R < n; g += nwaves) {  // (wave-uniform: every lane takes the cross-lane reads)
      const uint64_t r = g * R + rl;
      const bool live = rl < R && r < n;
      uint32_t key = kCmpAllEq;
      if (live) {
        const uint64_t c = r * cpr + q;
        const u32x4 va = a[c], vb = b[c];
        key = cmp_chunk_key(w, va, vb, 4u * q);
      }
      // segmented minimum over the record's cpr lanes, into its first lane
      for (uint32_t o = 1; o < cpr; o <<= 1) {
        const uint32_t y = __shfl_down(key, o, 64);
        if (q + o < cpr) key = min(key, y);
      }
      if (live && q == 0u) out[r] = cmp_result(key == kCmpAllEq ? R_EQ : (key & 3u));
    }
  } else {
    for (uint64_t r = wave; r < n; r += nwaves) {
      uint32_t key = kCmpAllEq;
      for (uint32_t q = lane; q < cpr; q += 64u) {
        cmp_word w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = prog[4u * q + i];
        const uint64_t c = r * cpr + q;
        const u32x4 va = a[c], vb = b[c];
        key = min(key, cmp_chunk_key(w, va, vb, 4u * q));
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) key = min(key, static_cast<uint32_t>(__shfl_xor(key, o, 64)));
      if (lane == 0u) out[r] = cmp_result(key == kCmpAllEq ? R_EQ : (key & 3u));
    }
  }
}

// ------------------------------------------------------------ walk: bytes
// la bytes at pa against lb bytes at pb (any alignment, every byte in
// bounds): 16 bytes a step, then 4, then the last 1..3; then the lengths.
__device__ __forceinline__ uint32_t cmp_bytes(const uint8_t *pa, const uint8_t *pb, uint32_t la, uint32_t lb) {
  const uint32_t m = min(la, lb);
  uint32_t i = 0;
  for (; i + 16u <= m; i += 16u) {
    const u32x4 x = ld16u(pa + i), y = ld16u(pb + i);
    if (x.x != y.x) return cmp_mem32(x.x, y.x);
    if (x.y != y.y) return cmp_mem32(x.y, y.y);
    if (x.z != y.z) return cmp_mem32(x.z, y.z);
    if (x.w != y.w) return cmp_mem32(x.w, y.w);
  }
  for (; i + 4u <= m; i += 4u) {
    const uint32_t x = ld32(pa + i), y = ld32(pb + i);
    if (x != y) return cmp_mem32(x, y);
  }
  for (; i < m; ++i) {
    const uint32_t x = pa[i], y = pb[i];
    if (x != y) return cmp_ord(x, y);
  }
  return cmp_ord(la, lb);
}

__device__ __forceinline__ uint64_t ld64u(const uint8_t *p) {
  return static_cast<uint64_t>(ld32(p)) | (static_cast<uint64_t>(ld32(p + 4)) << 32);
}
// [off, off + bytes) inside a heap of len bytes; an empty range reads
// nothing and is inside any heap
__device__ __forceinline__ bool ref_ok(uint64_t off, uint64_t bytes, uint64_t len) {
  return bytes == 0u || (off <= len && bytes <= len - off);
}
// A field that lies in the object itself (scalars, bool, enum, opaque[n]).
__device__ __forceinline__ uint32_t cmp_field(const xdrg_op &op, uint32_t cls, const uint8_t *ca,
                                              const uint8_t *cb) {
  switch (op.kind) {
  case XDRG_OP_U32: return cmp_w32(cls, ld32(ca + op.noff), ld32(cb + op.noff));
  case XDRG_OP_ENUM: return cmp_w32(XDRG_CLASS_SIGNED, ld32(ca + op.noff), ld32(cb + op.noff));
  case XDRG_OP_U64: return cmp_w64(cls, ld64u(ca + op.noff), ld64u(cb + op.noff));
  case XDRG_OP_BOOL: return cmp_ord(ca[op.noff] != 0, cb[op.noff] != 0);
  case XDRG_OP_OPAQUE: return cmp_bytes(ca + op.noff, cb + op.noff, op.arg0, op.arg0);
  default: return R_EQ;
  }
}

// The frames: reg_stack's (a's cursor in eb; dsum = the result the
// container's counts give once its common elements are equivalent) and,
// shifted with them, b's cursors.
struct cmp_stack {
  reg_stack st;
  uint64_t fb[kSubFrames];
  __device__ __forceinline__ void push(const sub_frame &x, uint64_t b) {
    st.push(0u, x);
#pragma unroll
    for (int j = kSubFrames - 1; j > 0; --j) fb[j] = fb[j - 1];
    fb[0] = b;
  }
  __device__ __forceinline__ void pop() {
    st.pop(0u);
#pragma unroll
    for (int j = 0; j + 1 < static_cast<int>(kSubFrames); ++j) fb[j] = fb[j + 1];
  }
};

// One lane, one pair: the records at ra and rb with their heaps.  ops and
// info are the plan's, in LDS when LDSOPS (cmp_lds_ops) or in global memory;
// info[pc] = class | (pc behind the union) << 8.  The walk of (a, b) follows
// the common path of the walks of (a, a) and (b, b): equal discriminants
// select the arm both took, a container compares min(count_a, count_b)
// elements.  xdrg_compare runs it once per pair, xdrg_sort (sort_kernels.h)
// as its comparator.
template <bool LDSOPS>
__device__ __forceinline__ int8_t cmp_walk_pair(const uint8_t *const ra, const uint8_t *const rb,
                                                const uint8_t *__restrict__ ah, uint64_t ahl,
                                                const uint8_t *__restrict__ bh, uint64_t bhl, const xdrg_op *ops,
                                                const uint32_t *info, const uint32_t *__restrict__ table) {
  const uint8_t *ca = ra, *cb = rb;  // the objects the walk is in: the records, or two elements
  cmp_stack S;
  uint32_t fp = 0, pc = 0;
  int8_t fin = XDRG_CMP_EQUAL;
  for (;;) {
    const xdrg_op op = LDSOPS ? ops[pc] : load_op(ops, pc);
    const uint32_t inf = info[pc];
    uint32_t res = R_EQ;
    if (op.kind == XDRG_OP_END) {
      if (fp == 0u) break;
      sub_frame &t = S.st.f[0];
      const xdrg_op v = LDSOPS ? ops[t.vpc()] : load_op(ops, t.vpc());
      if (t.left) {  // the next element pair
        --t.left;
        t.eb += v.arg1;
        S.fb[0] += v.arg1;
        ca = ah + t.eb;
        cb = bh + S.fb[0];
        pc = v.arg4;
        continue;
      }
      res = t.dsum;  // every common element equivalent: the counts decide
      pc = t.ret();
      S.pop();
      --fp;
      if (res != R_EQ) { fin = cmp_result(res); break; }
      ca = fp ? ah + S.st.f[0].eb : ra;
      cb = fp ? bh + S.fb[0] : rb;
      continue;
    }
    if (op.kind == XDRG_OP_JUMP) { pc = op.arg0; continue; }
    if (op.kind == XDRG_OP_UNION) {
      const uint32_t da = ld32(ca + op.noff), db = ld32(cb + op.noff);
      res = cmp_w32(inf & 0xffu, da, db);
      if (res != R_EQ) { fin = cmp_result(res); break; }
      const int t = union_target(op, table, da);
      pc = t < 0 ? inf >> 8 : static_cast<uint32_t>(t);  // no arm: equivalent, on behind the union
      continue;
    }
    if (op.kind == XDRG_OP_VAROPAQUE || op.kind == XDRG_OP_STRING) {
      const uint64_t oa = ld64u(ca + op.noff), ob = ld64u(cb + op.noff);
      const uint32_t la = ld32(ca + op.noff + 8), lb = ld32(cb + op.noff + 8);
      if (!ref_ok(oa, la, ahl) || !ref_ok(ob, lb, bhl)) { fin = XDRG_CMP_BADREF; break; }
      res = cmp_bytes(ah + oa, bh + ob, la, lb);
      if (res != R_EQ) { fin = cmp_result(res); break; }
      ++pc;
      continue;
    }
    if (op.kind == XDRG_OP_VECTOR) {
      const uint64_t oa = ld64u(ca + op.noff), ob = ld64u(cb + op.noff);
      const uint32_t na = ld32(ca + op.noff + 8), nb = ld32(cb + op.noff + 8);
      const uint64_t es = op.arg1;
      if (!ref_ok(oa, na * es, ahl) || !ref_ok(ob, nb * es, bhl)) { fin = XDRG_CMP_BADREF; break; }
      const uint32_t m = min(na, nb);
      const uint32_t after = cmp_ord(na, nb);  // the shorter container is less (absent < present)
      if (!(op.flags & XDRG_F_SUB)) {  // fixed-size elements: their ops inline
        for (uint32_t k = 0; k < m && res == R_EQ; ++k)
          for (uint32_t j = 0; j < op.arg2 && res == R_EQ; ++j) {
            const xdrg_op e = LDSOPS ? ops[pc + 1u + j] : load_op(ops, pc + 1u + j);
            res = cmp_field(e, info[pc + 1u + j] & 0xffu, ah + oa + k * es, bh + ob + k * es);
          }
        if (res == R_EQ) res = after;
        if (res != R_EQ) { fin = cmp_result(res); break; }
        pc += 1u + op.arg2;
        continue;
      }
      if (m == 0u) {
        if (after != R_EQ) { fin = cmp_result(after); break; }
        ++pc;
        continue;
      }
      if (S.st.lf >= XDRG_MAX_FRAMES) { fin = XDRG_CMP_DEEP; break; }  // (a cycle in a staged heap ends here)
      if (fp && S.st.f[0].left == 0u && sub_tail(ops, pc)) {
        // tail position: when this container closes so does the frame below;
        // take it over, with its return pc and, behind ours, its counts' result
        sub_frame &t = S.st.f[0];
        t = make_frame(oa, m - 1u, pc, t.ret(), after != R_EQ ? after : t.dsum, t.nf + 1u);
        S.fb[0] = ob;
      } else {
        if (fp == kSubFrames) { fin = XDRG_CMP_DEEP; break; }
        S.push(make_frame(oa, m - 1u, pc, pc + 1u, after, 1u), ob);
        ++fp;
      }
      ++S.st.lf;
      ca = ah + oa;
      cb = bh + ob;
      pc = op.arg4;
      continue;
    }
    res = cmp_field(op, inf & 0xffu, ca, cb);
    if (res != R_EQ) { fin = cmp_result(res); break; }
    ++pc;
  }
  return fin;
}

// The plan's ops and info into the workgroup's dynamic LDS (36 bytes per op),
// every lane of the workgroup calling; ends with a barrier.
__device__ __forceinline__ void cmp_lds_ops(const xdrg_op *__restrict__ g_ops, const uint32_t *__restrict__ g_info,
                                            uint32_t nops, const xdrg_op **ops, const uint32_t **info) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cmp_smem[];
  xdrg_op *sops = reinterpret_cast<xdrg_op *>(cmp_smem);
  uint32_t *sinfo = cmp_smem + 8u * nops;
  for (uint32_t i = threadIdx.x; i < nops; i += blockDim.x) sinfo[i] = g_info[i];
  load_ops(sops, g_ops, nops);  // (ends with the barrier)
  *ops = sops;
  *info = sinfo;
}

template <bool LDSOPS>
__global__ __launch_bounds__(256) void k_cmp_walk(const uint8_t *__restrict__ a, const uint8_t *__restrict__ ah,
                                                  uint64_t ahl, const uint8_t *__restrict__ b,
                                                  const uint8_t *__restrict__ bh, uint64_t bhl, uint64_t n,
                                                  uint32_t stride, const xdrg_op *__restrict__ g_ops,
                                                  const uint32_t *__restrict__ g_info, uint32_t nops,
                                                  const uint32_t *__restrict__ table, int8_t *__restrict__ out) {
  const xdrg_op *ops = g_ops;
  const uint32_t *info = g_info;
  if constexpr (LDSOPS) cmp_lds_ops(g_ops, g_info, nops, &ops, &info);
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n) return;
  out[r] = cmp_walk_pair<LDSOPS>(a + r * stride, b + r * stride, ah, ahl, bh, bhl, ops, info, table);
}

}  // namespace dev
}  // namespace xdrg
