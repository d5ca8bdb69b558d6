// Per-record decode verdicts (verify.hip): the decode's walk of one record
// with every check and no store, and the kernels built on it.
//
//   verify_walk   xdr_generic_get over one record [a, b) of the stream: the
//       checks of k_var_decode / sub_decode_rec (xdrgpu.hip, sub_kernels.h)
//       in their order -- stack budget, space, bounds, pads, validated enums,
//       discriminants -- returning (op << 8) | code of the first that fails,
//       0 when the record decodes.  It interprets the plan's ops, so one
//       walker serves fixed plans, var plans and element subroutines.  No
//       element area is allocated: the decode's area checks never decide a
//       record decoded alone (DESIGN.md "Per-record verdicts").
//   k_verify            one span per lane, the plan's ops in LDS.
//   k_rpc_verify_args   one dispatched call per lane, each with its own
//       procedure's plan (decode_arg, xdrpp/server.h:205-214); a failing
//       call becomes GARBAGE_ARGS in place (srpc.h:130-134).
//   k_gather_*          one procedure's argument bytes as an indexed stream.
//
// Frames.  An element subroutine's container opens a frame (elements left,
// the VECTOR op, the depth base to give back), kVerifyFrames per lane, kept
// in LDS ([frame][thread]: no private memory).  A container that is the last
// thing its body does and holds exactly one element opens none: its body's
// END is the enclosing body's END, so the walk adds the op's depth and
// jumps.  Pointer chains (rp__list) are verified at any length in no frame,
// bounded by the stack limit alone.  A record that needs more frames gets
// XDRG_ERR_INDEX_LONG at the VECTOR op that would open the next one: not
// decided here.
//
// Not embedded for hiprtc (build.py EMBED): the plan-specialized modules do
// not use it.
#pragma once
#include <type_traits>

#include "batch_kernels.h"
#include "elem_kernels.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kVerifyFrames = XDRG_INDEX_FRAMES;

__device__ __forceinline__ uint32_t verdict_of(uint32_t op, uint32_t code) {
  return ((op & 0xffffu) << 8) | code;
}

// Plan ops of a wave-uniform plan, staged in LDS (load_ops) ...
struct lds_ops {
  const xdrg_op *ops;
  __device__ __forceinline__ xdrg_op at(uint32_t pc) const { return ops[pc]; }
};
// ... or read where they lie: a lane's own plan (k_rpc_verify_args), or a
// plan too long for LDS.
struct glob_ops {
  const xdrg_op *ops;
  __device__ __forceinline__ xdrg_op at(uint32_t pc) const { return load_op(ops, pc); }
};

// kVerifyFrames frames of the calling lane: word (3 * f + k) of the lane at
// base[(3 * f + k) * nthreads], so a wave's accesses never share a bank.
struct lds_frames {
  static constexpr uint32_t kCap = kVerifyFrames;
  uint32_t *base;  // already offset by the thread's index
  uint32_t nthreads;
  __device__ __forceinline__ uint32_t &left(uint32_t f) { return base[(3u * f) * nthreads]; }
  __device__ __forceinline__ uint32_t &vpc(uint32_t f) { return base[(3u * f + 1u) * nthreads]; }
  __device__ __forceinline__ uint32_t &dsave(uint32_t f) { return base[(3u * f + 2u) * nthreads]; }
};
// Plans without element subroutines open no frame.
struct no_frames {
  static constexpr uint32_t kCap = 0;
  uint32_t none = 0;
  __device__ __forceinline__ uint32_t &left(uint32_t) { return none; }
  __device__ __forceinline__ uint32_t &vpc(uint32_t) { return none; }
  __device__ __forceinline__ uint32_t &dsave(uint32_t) { return none; }
};

// The op after `pc`, through jumps, is its body's END (sub_kernels.h sub_tail).
template <class OPS>
__device__ __forceinline__ bool verify_tail(const OPS &O, uint32_t pc) {
  xdrg_op q = O.at(pc + 1);
  while (q.kind == XDRG_OP_JUMP) q = O.at(q.arg0);
  return q.kind == XDRG_OP_END;
}

// One record [a, b) of the stream (4-byte aligned, a multiple of 4 long).
// Every read is of a word inside [a, b).
template <class OPS, class FR>
__device__ __forceinline__ uint32_t verify_walk(const OPS &O, const uint32_t *__restrict__ table,
                                                const uint8_t *__restrict__ xdr, uint64_t a, uint64_t b,
                                                uint32_t stack_limit, FR &fr) {
  uint64_t p = a;
  uint32_t fp = 0, pc = 0, dbase = 0;
  for (;;) {
    const xdrg_op op = O.at(pc);
    if (op.kind == XDRG_OP_END) {
      if (!fp) break;
      const uint32_t v = fr.vpc(fp - 1);
      if (fr.left(fp - 1)) {  // the container's next element
        --fr.left(fp - 1);
        const xdrg_op vo = O.at(v);
        dbase = fr.dsave(fp - 1) + vo.depth;
        pc = vo.arg4;
      } else {
        --fp;
        dbase = fr.dsave(fp);
        pc = v + 1;
      }
      continue;
    }
    if (op.kind == XDRG_OP_JUMP) { pc = op.arg0; continue; }
    if (static_cast<uint64_t>(dbase) + op.depth > stack_limit) return verdict_of(pc, XDRG_ERR_STACK_GET);
    const uint64_t rem = b - p;
    switch (op.kind) {
    case XDRG_OP_U32: case XDRG_OP_BOOL:
      if (rem < 4) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
      p += 4; ++pc; break;
    case XDRG_OP_ENUM: {
      if (rem < 4) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
      if ((op.flags & XDRG_F_VALIDATE) && !enum_ok(table, op.arg0, op.arg1, bswap32(ld32(xdr + p))))
        return verdict_of(pc, XDRG_ERR_INVALID_ENUM);
      p += 4; ++pc; break;
    }
    case XDRG_OP_U64:
      if (rem < 8) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
      p += 8; ++pc; break;
    case XDRG_OP_OPAQUE: {
      const uint32_t L = op.arg0;
      if (rem < L) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
      if ((L & 3u) && (ld32(xdr + p + (L & ~3u)) & ~keep_mask(L & 3u)))
        return verdict_of(pc, XDRG_ERR_NONZERO_PAD);
      p += (L + 3u) & ~3u; ++pc; break;
    }
    case XDRG_OP_VAROPAQUE: case XDRG_OP_STRING: {
      if (rem < 4) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
      const uint32_t L = bswap32(ld32(xdr + p));
      p += 4;
      if (L > b - p) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
      if (L > op.arg0)
        return verdict_of(pc, op.kind == XDRG_OP_STRING ? XDRG_ERR_XSTRING_BOUND : XDRG_ERR_XVECTOR_BOUND);
      if ((L & 3u) && (ld32(xdr + p + (L & ~3u)) & ~keep_mask(L & 3u)))
        return verdict_of(pc, XDRG_ERR_NONZERO_PAD);
      p += (static_cast<uint64_t>(L) + 3u) & ~3ull; ++pc; break;
    }
    case XDRG_OP_UNION: {
      if (rem < 4) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
      const uint32_t d = bswap32(ld32(xdr + p));
      p += 4;
      if ((op.flags & XDRG_F_VALIDATE) && !enum_ok(table, op.arg0, op.arg1, d))
        return verdict_of(pc, XDRG_ERR_INVALID_ENUM);
      const int t = union_target(op, table, d);
      if (t < 0) return verdict_of(pc, XDRG_ERR_BAD_DISCRIMINANT);
      pc = static_cast<uint32_t>(t);
      break;
    }
    case XDRG_OP_VECTOR: {
      if (rem < 4) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
      const uint32_t cnt = bswap32(ld32(xdr + p));
      p += 4;
      if (cnt > op.arg0)  // check_size (types.h:486-489, 605-608)
        return verdict_of(pc, (op.flags & XDRG_F_POINTER) ? XDRG_ERR_POINTER_BOUND : XDRG_ERR_XVECTOR_BOUND);
      if (op.flags & XDRG_F_SUB) {
        // every element takes at least arg3 wire bytes: a count the bytes
        // left cannot hold fails here, as in sub_decode_rec
        if (static_cast<uint64_t>(cnt) * op.arg3 > b - p) return verdict_of(pc, XDRG_ERR_OVERFLOW_GET);
        if (!cnt) { ++pc; break; }
        if (cnt == 1u && verify_tail(O, pc)) {  // tail container: no frame
          dbase += op.depth;
          pc = op.arg4;
          break;
        }
        if (fp == FR::kCap) return verdict_of(pc, XDRG_ERR_INDEX_LONG);
        fr.left(fp) = cnt - 1u;
        fr.vpc(fp) = pc;
        fr.dsave(fp) = dbase;
        ++fp;
        dbase += op.depth;
        pc = op.arg4;
        break;
      }
      // Inline elements, ops [pc + 1, pc + 1 + arg2), arg3 wire bytes each:
      // an element fails at its own op.  Elements with nothing to validate
      // (no pad bytes, no validated enum) are walked once, for the stack
      // budget; the rest are counted against the bytes left, and the one that
      // runs out is walked to find its op.
      const uint32_t nb = op.arg2, w = op.arg3;
      bool plain = true;
      for (uint32_t k = 1; k <= nb; ++k) {
        const xdrg_op e = O.at(pc + k);
        plain = plain && !(e.kind == XDRG_OP_ENUM && (e.flags & XDRG_F_VALIDATE)) &&
                !(e.kind == XDRG_OP_OPAQUE && (e.arg0 & 3u));
      }
      uint32_t left = cnt;
      bool first = true;
      while (left) {
        if (!first && plain) {
          const uint64_t m = min<uint64_t>(left, (b - p) / w);
          p += m * w;
          left -= static_cast<uint32_t>(m);
          if (!left) break;
        }
        for (uint32_t k = 1; k <= nb; ++k) {
          const xdrg_op e = O.at(pc + k);
          if (static_cast<uint64_t>(dbase) + e.depth > stack_limit) return verdict_of(pc + k, XDRG_ERR_STACK_GET);
          const uint32_t need = e.kind == XDRG_OP_U64 ? 8u : e.kind == XDRG_OP_OPAQUE ? e.arg0 : 4u;
          if (b - p < need) return verdict_of(pc + k, XDRG_ERR_OVERFLOW_GET);
          if (e.kind == XDRG_OP_OPAQUE) {
            if ((e.arg0 & 3u) && (ld32(xdr + p + (e.arg0 & ~3u)) & ~keep_mask(e.arg0 & 3u)))
              return verdict_of(pc + k, XDRG_ERR_NONZERO_PAD);
          } else if (e.kind == XDRG_OP_ENUM && (e.flags & XDRG_F_VALIDATE)) {
            if (!enum_ok(table, e.arg0, e.arg1, bswap32(ld32(xdr + p))))
              return verdict_of(pc + k, XDRG_ERR_INVALID_ENUM);
          }
          p += elem_wire_bytes(e);
        }
        --left;
        first = false;
      }
      pc += 1 + nb;
      break;
    }
    default: ++pc; break;
    }
  }
  return p != b ? verdict_of(kOpRecordLevel, XDRG_ERR_TRAILING) : 0u;
}

// The span's own checks, then the walk: what xdrg_decode reports for the
// record decoded alone (n = 1, offsets {a, b}).  A span whose start is not a
// multiple of 4 is refused like one outside the stream, and never read.
template <class OPS, class FR>
__device__ __forceinline__ uint32_t verify_span(const OPS &O, const uint32_t *__restrict__ table,
                                                const uint8_t *__restrict__ xdr, uint64_t len, uint64_t a,
                                                uint64_t b, uint32_t stack_limit, FR &fr) {
  if (b < a || b > len || (a & 3u)) return verdict_of(0, XDRG_ERR_OVERFLOW_GET);
  if ((b - a) & 3u) return verdict_of(kOpRecordLevel, XDRG_ERR_SIZE_NOT_MULT4);  // marshal.h:157-159
  return verify_walk(O, table, xdr, a, b, stack_limit, fr);
}

// LDS words a workgroup's frames take
__host__ __device__ inline uint32_t verify_frame_words(uint32_t nthreads) { return 3u * kVerifyFrames * nthreads; }

// One count of the wave's failed records (ballot + popcount).  Every lane of
// the wave must be active.
__device__ __forceinline__ void count_bad(unsigned long long *bad_count, bool bad) {
  const unsigned long long m = __ballot(bad);
  if (bad_count && m && __lane_id() == 0u) atomicAdd(bad_count, static_cast<unsigned long long>(__popcll(m)));
}

constexpr uint32_t kVerifyThreads = 256;     // plans without element subroutines
constexpr uint32_t kVerifySubThreads = 128;  // with: 24 KiB of frames a workgroup

// SUB: the plan has element subroutines (frames after the ops in LDS).
// LDSOPS: the ops fit in LDS.  stride8: u64 words between consecutive spans.
template <bool SUB, bool LDSOPS>
__global__ __launch_bounds__(SUB ? kVerifySubThreads : kVerifyThreads) void k_verify(
    const uint8_t *__restrict__ xdr, uint64_t len, const uint64_t *__restrict__ begin,
    const uint64_t *__restrict__ end, uint64_t stride8, uint64_t n, const xdrg_op *__restrict__ ops,
    uint32_t nops, const uint32_t *__restrict__ table, uint32_t stack_limit, uint32_t *__restrict__ verdicts,
    unsigned long long *bad_count) {
  extern __shared__ __attribute__((aligned(16))) uint32_t vsm[];
  uint32_t *fbase = vsm;
  if constexpr (LDSOPS) {
    load_ops(reinterpret_cast<xdrg_op *>(vsm), ops, nops);
    fbase = vsm + 8u * nops;
  }
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint32_t v = 0;
  if (r < n) {
    const uint64_t a = begin[r * stride8], b = end[r * stride8];
    using OPS = typename std::conditional<LDSOPS, lds_ops, glob_ops>::type;
    const OPS O{LDSOPS ? reinterpret_cast<const xdrg_op *>(vsm) : ops};
    if constexpr (SUB) {
      lds_frames fr{fbase + threadIdx.x, blockDim.x};
      v = verify_span(O, table, xdr, len, a, b, stack_limit, fr);
    } else {
      no_frames fr;
      v = verify_span(O, table, xdr, len, a, b, stack_limit, fr);
    }
    verdicts[r] = v;
  }
  count_bad(bad_count, v != 0u);
}

// ------------------------------------------------- RPC argument verdicts
// The plan table of one xdrg_rpc_verify_args call, a kernel argument (no
// upload per call): each procedure's device tables and its key.
struct verify_argplan {
  const xdrg_op *ops;
  const uint32_t *table;
  uint32_t nops, prog, vers, proc;
};
struct verify_argtable {
  verify_argplan e[XDRG_RPC_MAX_ARGPLANS];
};
static_assert(sizeof(verify_argplan) == 32, "64 plans are 2 KiB of kernel arguments");

// One header per lane.  A dispatched call whose procedure is in the table
// has its arguments [body_off, end) walked with that procedure's plan (the
// lanes of a wave hold different plans).  LDSOPS: every plan's ops are
// staged in LDS back to back, in table order (the host checked that they
// fit); else each lane reads its plan's ops where they lie.  The table is
// searched by a wave-uniform loop: its reads stay scalar.
template <bool SUB, bool LDSOPS>
__global__ __launch_bounds__(SUB ? kVerifySubThreads : kVerifyThreads) void k_rpc_verify_args(
    const uint8_t *__restrict__ xdr, uint64_t len, xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
    const verify_argtable T, uint32_t nplans, uint32_t stack_limit, uint32_t *__restrict__ verdicts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t vsm[];
  uint32_t *fbase = vsm;
  if constexpr (LDSOPS) {
    uint32_t at = 0;
    for (uint32_t i = 0; i < nplans; ++i) {
      const uint32_t *src = reinterpret_cast<const uint32_t *>(T.e[i].ops);
      for (uint32_t k = threadIdx.x; k < 8u * T.e[i].nops; k += blockDim.x) vsm[8u * at + k] = src[k];
      at += T.e[i].nops;
    }
    fbase = vsm + 8u * at;
    __syncthreads();
  }
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n) return;
  xdrg_rpc_hdr *h = hdrs + r;
  uint32_t v = 0;
  if (h->action == XDRG_RPC_DISPATCH) {
    const uint32_t P = h->w[XDRG_RPC_W_PROG], V = h->w[XDRG_RPC_W_VERS], Q = h->w[XDRG_RPC_W_PROC];
    const xdrg_op *ops = nullptr;
    const uint32_t *table = nullptr;
    uint32_t at = 0;
    for (uint32_t i = 0; i < nplans; ++i) {
      const bool hit = T.e[i].prog == P && T.e[i].vers == V && T.e[i].proc == Q;
      ops = hit ? (LDSOPS ? reinterpret_cast<const xdrg_op *>(vsm) + at : T.e[i].ops) : ops;
      table = hit ? T.e[i].table : table;
      at += T.e[i].nops;
    }
    if (ops) {
      const uint64_t a = h->body_off, b = h->end;
      using OPS = typename std::conditional<LDSOPS, lds_ops, glob_ops>::type;
      const OPS O{ops};
      if constexpr (SUB) {
        lds_frames fr{fbase + threadIdx.x, blockDim.x};
        v = verify_span(O, table, xdr, len, a, b, stack_limit, fr);
      } else {
        no_frames fr;
        v = verify_span(O, table, xdr, len, a, b, stack_limit, fr);
      }
      if (v) {  // decode_arg failed: GARBAGE_ARGS (srpc.h:130-134)
        h->action = XDRG_RPC_GARBAGE_ARGS;
        h->err = static_cast<uint8_t>(v & 0xffu);
      }
    }
  }
  if (verdicts) verdicts[r] = v;
}

// ---------------------------------------------------- RPC argument gather
// The headers a selector picks, in message order, as an indexed stream: per
// 256-header tile the count of selected headers and their body bytes
// (k_gather_count), the exclusive scan of both (k_tile_scan<2, 2,
// gather_totals>), then index, offsets and the bytes (k_gather_emit).  SEL is
// gather_key here, gather_res_key in replies_kernels.h.

// The calls of one procedure: dispatched, with the key's numbers.
struct gather_key {
  uint32_t prog, vers, proc;
  __device__ __forceinline__ bool operator()(const xdrg_rpc_hdr *h, uint64_t) const {
    return h->action == XDRG_RPC_DISPATCH && h->w[XDRG_RPC_W_PROG] == prog && h->w[XDRG_RPC_W_VERS] == vers &&
           h->w[XDRG_RPC_W_PROC] == proc;
  }
};

// Selected: a header K picks whose body lies inside the stream (a header with
// end < body_off or end > len is skipped: nothing of it is read).  *bytes =
// its body bytes.
template <class SEL>
__device__ __forceinline__ bool gather_sel(const SEL &K, const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t i,
                                           uint64_t n, uint64_t len, uint64_t *src, uint64_t *bytes) {
  *src = 0;
  *bytes = 0;
  if (i >= n || !K(hdrs + i, i)) return false;
  const uint64_t a = hdrs[i].body_off, b = hdrs[i].end;
  if (b < a || b > len) return false;
  *src = a;
  *bytes = b - a;
  return true;
}

template <class SEL>
__global__ __launch_bounds__(kTileThreads) void k_gather_count(const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n,
                                                               uint64_t len, const SEL K,
                                                               unsigned long long *__restrict__ tile_cnt,
                                                               unsigned long long *__restrict__ tile_bytes) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  uint64_t src, bytes;
  const bool sel = gather_sel(K, hdrs, i, n, len, &src, &bytes);
  tile_reduce(bytes, sel, tile_bytes, tile_cnt);
}

// Index and offsets a lane per header; the bytes a wave per run of 64
// headers: its selected bodies are one contiguous stretch of the output,
// written 4 bytes a lane per step (coalesced), each word's message found by
// stretch_find.  Bodies that are not whole aligned words (forged headers) go
// byte by byte the same way.  A body that does not fit the capacity is
// XDRG_ERR_OVERFLOW_PUT at its message (stretch_place).
template <class SEL>
__global__ __launch_bounds__(kTileThreads) void k_gather_emit(
    const uint8_t *__restrict__ xdr, uint64_t len, const xdrg_rpc_hdr *__restrict__ hdrs, uint64_t n, const SEL K,
    uint8_t *__restrict__ out, uint64_t cap, uint64_t *__restrict__ offsets, uint64_t *__restrict__ index,
    const unsigned long long *__restrict__ tile_cnt, const unsigned long long *__restrict__ tile_bytes,
    unsigned long long *err) {
  __shared__ unsigned long long wc[kTileThreads / 64];
  __shared__ unsigned long long s_end[kTileThreads], s_src[kTileThreads];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTileThreads + tid;
  uint64_t src, bytes;
  const bool sel = gather_sel(K, hdrs, i, n, len, &src, &bytes);
  const uint64_t ic = wave_incl_scan64(sel ? 1u : 0u);
  if (lane == 63u) wc[wid] = ic;  // read in put(), after stretch_place's barrier
  unsigned long long *w_end = s_end + 64u * wid, *w_src = s_src + 64u * wid;
  const stretch_at p = stretch_place(bytes, sel, i, tile_bytes, cap, err, w_end, [&](uint64_t at) {
    uint64_t k = tile_cnt[blockIdx.x] + ic - 1u;
    for (uint32_t w = 0; w < wid; ++w) k += wc[w];
    if (sel) {
      index[k] = i;
      offsets[k] = at;
    }
  });
  w_src[lane] = src;
  const bool words = __ballot(p.fits && ((src | bytes) & 3u)) == 0ull &&
                     !((reinterpret_cast<uintptr_t>(xdr) | (reinterpret_cast<uintptr_t>(out) + p.wbase)) & 3u);
  __syncthreads();
  const uint64_t total = w_end[63];
  const uint32_t unit = words ? 4u : 1u;
  for (uint64_t off = static_cast<uint64_t>(lane) * unit; off < total; off += 64u * unit) {
    const uint32_t m = stretch_find(w_end, off);
    const uint64_t start = m ? w_end[m - 1] : 0u;
    const uint8_t *s = xdr + w_src[m] + (off - start);
    uint8_t *d = out + p.wbase + off;
    if (words) st32(d, ld32(s));
    else *d = *s;
  }
}

}  // namespace dev
}  // namespace xdrg
