// Comparison of record batches on gfx950: the launchers of compare_kernels.h.
//
//   xdrg_plan_set_compare_classes  the value classes beside a plan's ops
//   xdrg_compare                   xdr::operator<=> / operator== per pair
//                                  (xdrpp/types.h:946-1062, :647-657)
//
// xdrg_compare validates its arguments on the host before the first HIP
// call, launches kernels only (no memset or memcpy nodes: xdrgpu.h "Graph
// capture") and keeps no state; the plan's first compare on a device uploads
// the class table and the word program (synchronously, as a plan's first
// launch uploads its tables).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "compare_host.h"
#include "compare_kernels.h"

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

namespace {

// The pc behind the union at u (where the walk goes on when equal
// discriminants select no arm).  Every non-void arm ends with a JUMP at the
// union's depth to that pc, and a void case's target is that pc.  M, the
// highest target, is either it (some JUMP of the union before M goes there,
// or the union has no arm ops at all) or the start of the last arm, whose
// own JUMP is the first one at the union's depth from M on -- an arm holds
// no UNION op at that depth (a nested one is a level deeper) and no op
// above it, which tells an arm from what follows an all-void union.
uint32_t union_end(const xdrg_plan &p, uint32_t u) {
  const xdrg_op &op = p.ops[u];
  uint32_t M = u + 1u;
  for (uint32_t c = 0; c < op.arg3; ++c) M = std::max(M, p.table[op.arg2 + 2u * c + 1u]);
  if (op.flags & XDRG_F_DEFAULT) M = std::max(M, op.arg4);
  for (uint32_t q = u + 1u; q < M && q < p.ops.size(); ++q)
    if (p.ops[q].kind == XDRG_OP_JUMP && p.ops[q].depth == op.depth && p.ops[q].arg0 == M) return M;
  for (uint32_t q = M; q < p.ops.size(); ++q) {
    const xdrg_op &e = p.ops[q];
    if (e.kind == XDRG_OP_JUMP && e.depth == op.depth) return e.arg0;
    if (e.kind == XDRG_OP_END || e.depth < op.depth || (e.kind == XDRG_OP_UNION && e.depth == op.depth)) break;
  }
  return M;
}

// The word program of k_cmp_fixed, when the plan is one it serves: a fixed
// plan (no references, no unions), stride a multiple of 16, fields at
// ascending, naturally aligned offsets (so word order is declaration order).
bool build_word_program(const xdrg_plan &p, const uint8_t *cls, std::vector<cmp_word> &prog) {
  if (p.path == XDRG_PATH_VAR || p.stride == 0u || (p.stride & 15u)) return false;
  prog.assign(p.stride / 4u, cmp_word{CW_PAD, 0u, 0u, 0u});
  uint64_t next = 0;  // first byte past the fields so far
  for (size_t i = 0; i < p.ops.size(); ++i) {
    const xdrg_op &op = p.ops[i];
    if (op.kind == XDRG_OP_END) break;
    uint32_t size;
    switch (op.kind) {
    case XDRG_OP_U32: case XDRG_OP_ENUM: size = 4; break;
    case XDRG_OP_U64: size = 8; break;
    case XDRG_OP_BOOL: size = 1; break;
    case XDRG_OP_OPAQUE: size = op.arg0; break;
    default: return false;
    }
    if (op.noff < next || uint64_t(op.noff) + size > p.stride) return false;
    next = uint64_t(op.noff) + size;
    const uint32_t w = op.noff / 4u;
    const uint32_t c = op.kind == XDRG_OP_ENUM ? uint32_t(XDRG_CLASS_SIGNED) : cls[i];
    if (op.kind == XDRG_OP_U32 || op.kind == XDRG_OP_ENUM) {
      if ((op.noff & 3u) || prog[w].kind != CW_PAD) return false;
      prog[w].kind = c == XDRG_CLASS_SIGNED ? CW_S32 : c == XDRG_CLASS_IEEE ? CW_F32 : CW_U32;
    } else if (op.kind == XDRG_OP_U64) {
      if ((op.noff & 7u) || prog[w].kind != CW_PAD) return false;  // both halves in one chunk
      prog[w].kind = c == XDRG_CLASS_SIGNED ? CW_S64 : c == XDRG_CLASS_IEEE ? CW_F64 : CW_U64;
    } else {
      for (uint32_t k = 0; k < size; ++k) {
        cmp_word &x = prog[(op.noff + k) / 4u];
        if (x.kind != CW_PAD && x.kind != CW_BYTES) return false;
        x.kind = CW_BYTES;
        (op.kind == XDRG_OP_BOOL ? x.bools : x.bytes) |= 0xffu << (8u * ((op.noff + k) & 3u));
      }
    }
  }
  return true;
}

bool needs_classes(const xdrg_plan &p) {
  for (const xdrg_op &op : p.ops)
    if (op.kind == XDRG_OP_U32 || op.kind == XDRG_OP_U64 || op.kind == XDRG_OP_UNION) return true;
  return false;
}

void install_classes(xdrg_plan &p, const uint8_t *cls) {
  p.cmp_info.assign(p.ops.size(), 0u);
  for (uint32_t i = 0; i < p.ops.size(); ++i)
    p.cmp_info[i] = cls[i] | (p.ops[i].kind == XDRG_OP_UNION ? union_end(p, i) << 8 : 0u);
  p.cmp_fixed = build_word_program(p, cls, p.cmp_prog);
  if (!p.cmp_fixed) p.cmp_prog.clear();
  p.has_cmp = true;
}

constexpr uint32_t kCmpMaxBlocks = 1u << 22;  // past it the chunk kernel's waves loop

}  // namespace

namespace xdrg {
namespace host {

int cmp_upload(const xdrg_plan *cp, cmp_tables *out) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) return XDRG_EUNSUPPORTED;
  xdrg_plan *p = const_cast<xdrg_plan *>(cp);
  const size_t info_bytes = align256(p->cmp_info.size() * 4u);
  if (!p->cmp_uploaded[dev].load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> g(p->upload_mu);
    if (!p->cmp_uploaded[dev].load(std::memory_order_relaxed)) {
      void *mem = nullptr;
      HIPCHK(hipMalloc(&mem, info_bytes + align256(p->cmp_prog.size() * sizeof(cmp_word)) + 256u));
      hipError_t e = hipMemcpy(mem, p->cmp_info.data(), p->cmp_info.size() * 4u, hipMemcpyHostToDevice);
      if (e == hipSuccess && !p->cmp_prog.empty())
        e = hipMemcpy(static_cast<char *>(mem) + info_bytes, p->cmp_prog.data(),
                      p->cmp_prog.size() * sizeof(cmp_word), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        (void)hipFree(mem);
        return record_hip_error(int(e), "hipMemcpy(compare tables)");
      }
      p->cmp_dev[dev] = mem;
      p->cmp_uploaded[dev].store(true, std::memory_order_release);
    }
  }
  out->d_info = static_cast<const uint32_t *>(p->cmp_dev[dev]);
  out->d_prog = reinterpret_cast<const cmp_word *>(static_cast<const char *>(p->cmp_dev[dev]) + info_bytes);
  return XDRG_OK;
}

int cmp_classes_ready(const xdrg_plan *plan) {
  if (plan->has_cmp) return XDRG_OK;
  if (needs_classes(*plan)) return XDRG_EUNSUPPORTED;
  // nothing to classify (bools, enums, bytes): every class is 0
  std::lock_guard<std::mutex> g(const_cast<xdrg_plan *>(plan)->upload_mu);
  if (!plan->has_cmp) {
    const std::vector<uint8_t> zero(plan->ops.size(), 0);
    install_classes(*const_cast<xdrg_plan *>(plan), zero.data());
  }
  return XDRG_OK;
}

}  // namespace host
}  // namespace xdrg

extern "C" {

int xdrg_plan_set_compare_classes(xdrg_plan *plan, const uint8_t *classes, uint32_t nops) {
  if (!plan || !classes || nops != plan->ops.size()) return XDRG_EINVAL;
  for (uint32_t i = 0; i < nops; ++i) {
    const uint32_t top = plan->ops[i].kind == XDRG_OP_UNION ? XDRG_CLASS_BOOL : XDRG_CLASS_IEEE;
    if (classes[i] > top || (plan->ops[i].kind == XDRG_OP_UNION && classes[i] == XDRG_CLASS_IEEE))
      return XDRG_EINVAL;
  }
  for (int d = 0; d < kMaxDevices; ++d)
    if (plan->cmp_uploaded[d].load()) return XDRG_EINVAL;  // (set before the plan's first compare)
  install_classes(*plan, classes);
  return XDRG_OK;
}

int xdrg_compare(const xdrg_plan *plan, const void *d_a, const void *d_a_heap, uint64_t a_heap_len,
                 const void *d_b, const void *d_b_heap, uint64_t b_heap_len, uint64_t n, int8_t *d_result,
                 void *stream) {
  if (!plan || (n && (!d_a || !d_b || !d_result))) return XDRG_EINVAL;
  if ((!d_a_heap && a_heap_len) || (!d_b_heap && b_heap_len)) return XDRG_EINVAL;
  const bool var = plan->path == XDRG_PATH_VAR;
  if (misaligned(d_a, var ? 7 : 3) || misaligned(d_b, var ? 7 : 3) || misaligned(d_a_heap, 3) ||
      misaligned(d_b_heap, 3))
    return XDRG_EALIGN;
  int rc = cmp_classes_ready(plan);
  if (rc != XDRG_OK) return rc;
  if (n == 0) return XDRG_OK;
  const uint32_t nops = uint32_t(plan->ops.size());
  const bool chunks = plan->cmp_fixed && !misaligned(d_a, 15) && !misaligned(d_b, 15);
  const uint64_t walk_blocks = (n + 255u) / 256u;
  if (!chunks && walk_blocks > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  const dev_tables *T = nullptr;
  rc = plan_tables(plan, &T);
  if (rc != XDRG_OK) return rc;
  cmp_tables C = {};
  rc = cmp_upload(plan, &C);
  if (rc != XDRG_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (chunks) {
    const uint32_t cpr = plan->stride / 16u;
    const u32x4 *a = static_cast<const u32x4 *>(d_a), *b = static_cast<const u32x4 *>(d_b);
    if (cpr <= 64u) {
      const uint64_t R = 64u / cpr, waves = (n + R - 1) / R;
      const uint32_t nb = uint32_t(std::min<uint64_t>((waves + 3) / 4, kCmpMaxBlocks));
      k_cmp_fixed<false><<<nb, 256, 0, s>>>(a, b, n, cpr, C.d_prog, d_result);
    } else {
      const uint32_t nb = uint32_t(std::min<uint64_t>((n + 3) / 4, kCmpMaxBlocks));
      k_cmp_fixed<true><<<nb, 256, 0, s>>>(a, b, n, cpr, C.d_prog, d_result);
    }
  } else {
    const uint8_t *a = static_cast<const uint8_t *>(d_a), *b = static_cast<const uint8_t *>(d_b);
    const uint8_t *ah = static_cast<const uint8_t *>(d_a_heap), *bh = static_cast<const uint8_t *>(d_b_heap);
    const size_t lds = size_t(nops) * (sizeof(xdrg_op) + 4u);
    if (lds <= kCmpLdsOps)
      k_cmp_walk<true><<<uint32_t(walk_blocks), 256, lds, s>>>(a, ah, a_heap_len, b, bh, b_heap_len, n, plan->stride,
                                                               T->d_ops, C.d_info, nops, T->d_table, d_result);
    else
      k_cmp_walk<false><<<uint32_t(walk_blocks), 256, 0, s>>>(a, ah, a_heap_len, b, bh, b_heap_len, n, plan->stride,
                                                              T->d_ops, C.d_info, nops, T->d_table, d_result);
  }
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

}  // extern "C"
