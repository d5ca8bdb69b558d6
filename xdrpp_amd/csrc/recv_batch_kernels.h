// The receive batch (recv_batch.hip, xdrg_rpc_recv_batch): many connections'
// receive buffers framed in one call, msg_sock::input per connection
// (xdrpp/msgsock.cc:38-119) with rpc_sock::recv_msg's test (msgsock.cc:202-225).
//
// count -> k_tile_scan -> emit over tiles of 256 connections, each pass in two
// kernels because both regimes are real (a million connections of one message,
// one connection of a million messages):
//
//   lane pass   k_rb_count / k_rb_emit: one lane per connection.  A connection
//               of at most kRbLaneBytes is walked by its lane, mark by mark,
//               straight from global memory (the 64 segments of a wave lie
//               next to each other, so its lanes share cache lines); a longer
//               one is appended to a list (k_rb_count) and left to the wave
//               pass.  k_rb_emit also gives every connection, listed or not,
//               its first message and its base in the stream: the tile's base
//               from the scan and the connections before it in the tile.
//   wave pass   k_rb_count_wave / k_rb_emit_wave: one single-wave workgroup per
//               listed connection walks it through LDS windows of kRbWinBytes,
//               loaded with 16-byte loads; the chain is followed as uniform
//               (scalar) work, one LDS read per message, and a message longer
//               than the window moves the next load to the next mark, so long
//               bodies are never read by the walk.
//   copy        k_rb_copy: the delivered messages of a connection are a prefix
//               of its segment, so the stream is the concatenation of these
//               prefixes: aligned 16-byte lines of d_out, each finding its
//               connection by a binary search of the bases.
//
// The walk is deterministic, so the emit repeats it and nothing is logged.
// Whatever the table holds, rb_seg clamps a segment into [0, buf_len), every
// message index is tested against max_msgs and every output byte against the
// capacity before it is written.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_kernels.h"

namespace xdrg {
namespace dev {

constexpr uint32_t kRbLaneBytes = 1024;   // a longer connection goes to the wave pass
constexpr uint32_t kRbWinBytes = 16384;   // LDS window of the wave pass
constexpr uint32_t kRbWaveGrid = 4096;    // workgroups of the wave pass, at most
constexpr uint32_t kRbCopyGrid = 2048;    // workgroups of the copy, at most

static_assert(sizeof(xdrg_rpc_conn) == 32 && sizeof(xdrg_rpc_conn_in) == 16, "xdrgpu.h: the receive batch");

// What the stage keeps between its kernels besides the tile words.
struct rb_ctl {
  uint32_t listed, rsv;          // connections left to the wave pass (k_fill32: 0)
  unsigned long long fit;        // start of the first message that does not fit d_out (k_fill32: ~0)
};

struct rb_args {
  const uint8_t *buf;
  uint64_t buf_len;
  const xdrg_rpc_conn_in *segs;
  uint64_t nconns;
  uint32_t maxlen, rpc;
};

struct rb_outs {
  uint64_t *offsets;
  uint64_t max_msgs, cap;
  uint32_t *conn_of;
  uint8_t *kind;
  unsigned long long *err;
  rb_ctl *ctl;
};

// Connection c's bytes, clamped: a 4-aligned start inside the buffer and a
// length that ends inside it, whatever the table says.
__device__ __forceinline__ void rb_seg(const rb_args &A, uint64_t c, uint64_t *b, uint64_t *l) {
  const xdrg_rpc_conn_in s = A.segs[c];
  const uint64_t top = A.buf_len & ~3ull;
  *b = (s.begin < top ? s.begin : top) & ~3ull;
  *l = s.len < A.buf_len - *b ? s.len : A.buf_len - *b;
}

// One mark of a connection whose segment has `rem` bytes left from it, in
// ix_mark's order (xdrgpu.hip, read_message srpc.cc:29-55 with msg_sock's
// length rule); rem == 0 and the two EOFs leave the connection open.
//   premature EOF on the mark        OPEN, need 4      msgsock.cc:68-81 (rdpos_ < 4)
//   pre-swap size test (raw & 3)     BAD_SIZE          srpc.cc:38-39
//   last-fragment bit clear          FRAGMENT          msgsock.cc:86-91
//   size > maxmsglen_                TOO_LONG          msgsock.cc:99-117, from the mark alone
//   body ends past the segment       OPEN, need 4 + size   msgsock.cc:43-66 (rdmsg_, rdpos_)
//   size not a multiple of 4         BAD_SIZE          marshal.h:152-162
// Returns true for a whole message of *size body bytes.
__device__ __forceinline__ bool rb_mark(uint32_t raw, uint64_t rem, uint32_t maxlen, uint32_t *size, uint32_t *state,
                                        uint32_t *need) {
  *state = XDRG_CONN_OPEN;
  *need = 0;
  if (rem == 0) return false;
  if (rem < 4) { *need = 4; return false; }
  if (raw & 3u) { *state = XDRG_CONN_BAD_SIZE; return false; }
  const uint32_t v = bswap32(raw);
  if (!(v & XDRG_MARK_LAST)) { *state = XDRG_CONN_FRAGMENT; return false; }
  const uint32_t sz = v & ~XDRG_MARK_LAST;
  if (sz > maxlen) { *state = XDRG_CONN_TOO_LONG; return false; }
  if (rem - 4 < sz) { *need = 4u + sz; return false; }
  if (sz & 3u) { *state = XDRG_CONN_BAD_SIZE; return false; }
  *size = sz;
  return true;
}

// rpc_sock::recv_msg's test of a whole message (msgsock.cc:205-224): at least
// 8 bytes, word 1 BE(CALL) or BE(REPLY).  w1: the raw word.
__device__ __forceinline__ bool rb_rpc_ok(uint32_t size, uint32_t w1) {
  return size >= 8u && (w1 == 0u || w1 == 0x01000000u);
}

struct rb_result {
  uint64_t consumed, msgs;
  uint32_t need, state;
};

__device__ __forceinline__ void rb_store(xdrg_rpc_conn *conns, uint64_t c, const rb_result &r) {
  conns[c].consumed = r.consumed;
  conns[c].msgs = r.msgs;
  conns[c].need = r.need;
  conns[c].state = r.state;
}

// Message k of the batch starts at `at` and has `bytes` with its mark.
__device__ __forceinline__ void rb_put(const rb_outs &O, uint64_t k, uint64_t at, uint64_t bytes, uint32_t conn,
                                       uint32_t kind) {
  if (k <= O.max_msgs) O.offsets[k] = at;  // k == max_msgs: where the messages that were indexed end
  if (k < O.max_msgs) {
    O.conn_of[k] = conn;
    if (O.kind) O.kind[k] = static_cast<uint8_t>(kind);
  }
  if (at <= O.cap && bytes > O.cap - at) {  // the first that does not fit: the ones after it start past the capacity
    O.ctl->fit = at;
    report(O.err, k, kOpRecordLevel, XDRG_ERR_OVERFLOW_PUT);  // xdr_generic_put::check (marshal.h:104-108)
  }
}

// The walk of one lane over its connection, from global memory.  EMIT: O,
// first and base are used.
template <bool EMIT>
__device__ __forceinline__ rb_result rb_lane_walk(const rb_args &A, const uint8_t *s, uint64_t l, const rb_outs &O,
                                                  uint64_t first, uint64_t base, uint32_t conn) {
  rb_result r{0, 0, 0, XDRG_CONN_OPEN};
  for (;;) {
    const uint64_t rem = l - r.consumed;
    uint32_t size = 0;
    if (!rb_mark(rem >= 4 ? ld32(s + r.consumed) : 0u, rem, A.maxlen, &size, &r.state, &r.need)) break;
    uint32_t kind = 0;
    if (A.rpc) {
      const uint32_t w1 = size >= 8u ? ld32(s + r.consumed + 8) : 0u;
      if (!rb_rpc_ok(size, w1)) { r.state = XDRG_CONN_BAD_RPC; break; }
      kind = w1 != 0u;
    }
    if constexpr (EMIT) rb_put(O, first + r.msgs, base + r.consumed, 4ull + size, conn, kind);
    r.consumed += 4ull + size;
    ++r.msgs;
  }
  return r;
}

// The two sums of a tile: every lane of the kTileThreads must call.
__device__ __forceinline__ void rb_tile_sums(unsigned long long m, unsigned long long b,
                                             unsigned long long *__restrict__ tile_msgs,
                                             unsigned long long *__restrict__ tile_bytes) {
  __shared__ unsigned long long ws[2][kTileThreads / 64];
  for (int o = 32; o > 0; o >>= 1) {
    m += __shfl_xor(m, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
    ws[0][threadIdx.x >> 6] = m;
    ws[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sm = 0, sb = 0;
    for (uint32_t k = 0; k < kTileThreads / 64; ++k) {
      sm += ws[0][k];
      sb += ws[1][k];
    }
    tile_msgs[blockIdx.x] = sm;
    tile_bytes[blockIdx.x] = sb;
  }
}

// ------------------------------------------------------------- lane pass
template <class = void>
__global__ __launch_bounds__(kTileThreads) void k_rb_count(const rb_args A, xdrg_rpc_conn *__restrict__ conns,
                                                           unsigned long long *__restrict__ tile_msgs,
                                                           unsigned long long *__restrict__ tile_bytes,
                                                           uint32_t *__restrict__ list, rb_ctl *__restrict__ ctl) {
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  rb_result r{0, 0, 0, XDRG_CONN_OPEN};
  if (c < A.nconns) {
    uint64_t b, l;
    rb_seg(A, c, &b, &l);
    if (l > kRbLaneBytes) {
      list[atomicAdd(&ctl->listed, 1u)] = static_cast<uint32_t>(c);  // its sums: k_rb_count_wave
    } else {
      r = rb_lane_walk<false>(A, A.buf + b, l, rb_outs{}, 0, 0, 0);
      rb_store(conns, c, r);
    }
  }
  rb_tile_sums(r.msgs, r.consumed, tile_msgs, tile_bytes);
}

template <class = void>
__global__ __launch_bounds__(kTileThreads) void k_rb_emit(const rb_args A, xdrg_rpc_conn *__restrict__ conns,
                                                          const unsigned long long *__restrict__ tile_msgs,
                                                          const unsigned long long *__restrict__ tile_bytes,
                                                          unsigned long long *__restrict__ cbase, const rb_outs O) {
  __shared__ unsigned long long wm[kTileThreads / 64], wb[kTileThreads / 64];
  const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kTileThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const bool in = c < A.nconns;
  const uint64_t msgs = in ? conns[c].msgs : 0u, bytes = in ? conns[c].consumed : 0u;
  const uint64_t im = wave_incl_scan64(msgs), ib = wave_incl_scan64(bytes);
  if (lane == 63u) {
    wm[wid] = im;
    wb[wid] = ib;
  }
  __syncthreads();
  uint64_t first = tile_msgs[blockIdx.x] + im - msgs, base = tile_bytes[blockIdx.x] + ib - bytes;
  for (uint32_t k = 0; k < wid; ++k) {
    first += wm[k];
    base += wb[k];
  }
  if (!in) return;
  conns[c].first = first;
  cbase[c] = base;
  uint64_t b, l;
  rb_seg(A, c, &b, &l);
  if (l <= kRbLaneBytes) rb_lane_walk<true>(A, A.buf + b, l, O, first, base, static_cast<uint32_t>(c));
}

// ------------------------------------------------------------- wave pass
// A value every lane holds, as a scalar: what is computed from it stays in
// scalar registers and branches on it are scalar branches.
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return static_cast<uint64_t>(uni32(static_cast<uint32_t>(v))) |
         (static_cast<uint64_t>(uni32(static_cast<uint32_t>(v >> 32))) << 32);
}

constexpr uint32_t kRbWinWords = kRbWinBytes / 4 + 4;  // word 1 of a message is read with its mark: room past the end

// The window: bytes [pos, pos + wlen) of the segment, wlen a multiple of 4.
// Every 16-byte load of the window is in flight before the first LDS store
// (16 a lane): one memory round trip a window.
__device__ __forceinline__ uint32_t rb_win_load(uint32_t *win, const uint8_t *s, uint64_t l, uint64_t pos,
                                                uint32_t lane) {
  constexpr int UL = kRbWinBytes / 16 / 64;
  const uint64_t left = (l - pos) & ~3ull;
  const uint32_t wlen = left < kRbWinBytes ? static_cast<uint32_t>(left) : kRbWinBytes;
  const uint8_t *src = s + pos;
  const uint32_t n16 = wlen / 16u;
  u32x4 t[UL];
#pragma unroll
  for (int k = 0; k < UL; ++k) {
    const uint32_t i = 64u * k + lane;
    if (i < n16) t[k] = ld16u(src + 16u * i);
  }
#pragma unroll
  for (int k = 0; k < UL; ++k) {
    const uint32_t i = 64u * k + lane;
    if (i < n16) reinterpret_cast<u32x4 *>(win)[i] = t[k];
  }
  for (uint32_t i = n16 * 4u + lane; i < wlen / 4u; i += 64u) win[i] = ld32(src + 4u * i);
  wave_sync();
  return wlen;
}

// One wave walks one connection.  Every value of the walk is uniform
// (uni32 of the window's words), so the chain is scalar work.  EMIT:
// lane j keeps message 64 q + j, and the wave writes 64 entries at a time.
template <bool EMIT>
__device__ __forceinline__ rb_result rb_wave_walk(const rb_args &A, uint32_t *win, const uint8_t *s, uint64_t l,
                                                  const rb_outs &O, uint64_t first, uint64_t base, uint32_t conn,
                                                  uint32_t lane) {
  rb_result r{0, 0, 0, XDRG_CONN_OPEN};
  uint64_t w0 = 0, my_at = 0, my_bytes = 0;
  uint32_t wlen = 0, my_kind = 0;
  bool loaded = false;
  for (;;) {
    const uint64_t pos = r.consumed, rem = l - pos;
    // the mark and, for recv_msg's test, word 1 of the message: up to 12 bytes from pos
    const uint64_t want = rem < 12u ? rem & ~3ull : 12u;
    if (!loaded || pos < w0 || pos + want > w0 + wlen) {
      wave_sync();  // the reads of the window before it is overwritten
      wlen = rb_win_load(win, s, l, pos, lane);
      w0 = pos;
      loaded = true;
    }
    const uint32_t wi = static_cast<uint32_t>(pos - w0) >> 2;  // at most kRbWinBytes / 4
    uint32_t size = 0;
    // the mark and word 1 in one LDS round trip; either is used only where the window holds it
    const uint32_t raw = uni32(win[wi]), w1 = uni32(win[wi + 2]);
    if (!rb_mark(rem >= 4 ? raw : 0u, rem, A.maxlen, &size, &r.state, &r.need)) break;
    uint32_t kind = 0;
    if (A.rpc) {
      if (!rb_rpc_ok(size, size >= 8u ? w1 : 0u)) { r.state = XDRG_CONN_BAD_RPC; break; }
      kind = w1 != 0u;
    }
    if constexpr (EMIT) {
      const uint32_t j = static_cast<uint32_t>(r.msgs) & 63u;
      if (lane == j) {
        my_at = base + pos;
        my_bytes = 4ull + size;
        my_kind = kind;
      }
      if (j == 63u) rb_put(O, first + r.msgs - 63u + lane, my_at, my_bytes, conn, my_kind);
    }
    r.consumed += 4ull + size;
    ++r.msgs;
  }
  if constexpr (EMIT) {
    const uint32_t tail = static_cast<uint32_t>(r.msgs) & 63u;
    if (lane < tail) rb_put(O, first + r.msgs - tail + lane, my_at, my_bytes, conn, my_kind);
  }
  return r;
}

// The listed connections' results, and their sums into the tile words the
// lane pass wrote (integer atomics: the sums do not depend on the order).
template <class = void>
__global__ __launch_bounds__(64) void k_rb_count_wave(const rb_args A, xdrg_rpc_conn *__restrict__ conns,
                                                      unsigned long long *__restrict__ tile_msgs,
                                                      unsigned long long *__restrict__ tile_bytes,
                                                      const uint32_t *__restrict__ list, const rb_ctl *__restrict__ ctl) {
  __shared__ __attribute__((aligned(16))) uint32_t win[kRbWinWords];
  const uint32_t lane = threadIdx.x;
  const uint64_t listed = ctl->listed < A.nconns ? ctl->listed : A.nconns;
  for (uint64_t i = blockIdx.x; i < listed; i += gridDim.x) {
    const uint64_t c = uni32(list[i]);
    if (c >= A.nconns) continue;
    uint64_t b, l;
    rb_seg(A, c, &b, &l);
    b = uni64(b);
    l = uni64(l);
    const rb_result r = rb_wave_walk<false>(A, win, A.buf + b, l, rb_outs{}, 0, 0, 0, lane);
    if (lane == 0) {
      rb_store(conns, c, r);
      atomicAdd(tile_msgs + c / kTileThreads, static_cast<unsigned long long>(r.msgs));
      atomicAdd(tile_bytes + c / kTileThreads, static_cast<unsigned long long>(r.consumed));
    }
  }
}

template <class = void>
__global__ __launch_bounds__(64) void k_rb_emit_wave(const rb_args A, const xdrg_rpc_conn *__restrict__ conns,
                                                     const unsigned long long *__restrict__ cbase,
                                                     const uint32_t *__restrict__ list, const rb_outs O) {
  __shared__ __attribute__((aligned(16))) uint32_t win[kRbWinWords];
  const uint32_t lane = threadIdx.x;
  const uint64_t listed = O.ctl->listed < A.nconns ? O.ctl->listed : A.nconns;
  for (uint64_t i = blockIdx.x; i < listed; i += gridDim.x) {
    const uint64_t c = uni32(list[i]);
    if (c >= A.nconns) continue;
    uint64_t b, l;
    rb_seg(A, c, &b, &l);
    rb_wave_walk<true>(A, win, A.buf + uni64(b), uni64(l), O, uni64(conns[c].first), uni64(cbase[c]),
                       static_cast<uint32_t>(c), lane);
  }
}

// ------------------------------------------------------------------- scan
// The totals: what gather_totals writes, bounded by max_msgs; more messages
// than that is XDRG_ERR_MSG_COUNT at record max_msgs (as xdrg_index_msgs).
struct rb_totals {
  uint64_t *count, *offsets;
  uint64_t max_msgs;
  xdrg_status *status;
  __device__ void operator()(const unsigned long long (&t)[2], uint32_t lane) const {
    if (lane) return;
    const uint64_t n = t[0] < max_msgs ? t[0] : max_msgs;
    *count = n;
    if (t[0] <= max_msgs) offsets[n] = t[1];  // else k_rb_emit writes offsets[max_msgs]
    else report(reinterpret_cast<unsigned long long *>(&status->first_error), max_msgs, kOpRecordLevel,
                XDRG_ERR_MSG_COUNT);
    status->total_bytes = t[1];
  }
};

// ------------------------------------------------------------------- copy
// Bytes [0, min(total, fit)) of the stream, an aligned 16-byte line of d_out
// a lane.  total: tile_bytes' last word after the scan is not kept, so the
// copy reads the end from the last connection's base and bytes.
template <class = void>
__global__ __launch_bounds__(256) void k_rb_copy(const rb_args A, const xdrg_rpc_conn *__restrict__ conns,
                                                 const unsigned long long *__restrict__ cbase,
                                                 const rb_ctl *__restrict__ ctl, uint8_t *__restrict__ out,
                                                 uint64_t cap) {
  const uint64_t total = cbase[A.nconns - 1] + conns[A.nconns - 1].consumed;
  uint64_t end = total < ctl->fit ? total : ctl->fit;
  if (end > cap) end = cap;  // never taken: fit <= cap whenever total > cap
  const uint64_t pre = reinterpret_cast<uintptr_t>(out) & 15u;
  const uint64_t nlines = end ? (pre + end + 15u) >> 4 : 0u;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nlines; i += stride) {
    const uint64_t lo = 16u * i < pre ? 0u : 16u * i - pre;  // stream bytes [lo, hi) of this line
    const uint64_t hi = 16u * i + 16u - pre < end ? 16u * i + 16u - pre : end;
    // the last connection whose base is at or before lo: the ones before it with the same base are empty
    uint64_t a = 0, z = A.nconns - 1;
    while (a < z) {
      const uint64_t mid = (a + z + 1) >> 1;
      if (cbase[mid] <= lo) a = mid; else z = mid - 1;
    }
    uint64_t c = a, cb = cbase[c], ce = cb + conns[c].consumed, sb, sl;
    rb_seg(A, c, &sb, &sl);
    if (hi - lo == 16u && hi <= ce) {  // a whole line of one connection
      *reinterpret_cast<u32x4 *>(out + lo) = ld16u(A.buf + sb + (lo - cb));
      continue;
    }
    for (uint64_t o = lo; o < hi; o += 4) {
      while (o >= ce && c + 1 < A.nconns) {
        ++c;
        cb = cbase[c];
        ce = cb + conns[c].consumed;
        rb_seg(A, c, &sb, &sl);
      }
      if (o < ce) st32(out + o, ld32(A.buf + sb + (o - cb)));
    }
  }
}

}  // namespace dev
}  // namespace xdrg
