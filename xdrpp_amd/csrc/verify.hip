// Per-record decode verdicts and batched RPC argument decoding on gfx950:
// the launchers of verify_kernels.h.
//
//   xdrg_verify            the decode walk without stores, one verdict per
//                          record (what xdrg_decode reports for the record
//                          decoded alone)
//   xdrg_rpc_verify_args   decode_arg (xdrpp/server.h:205-214) for a whole
//                          dispatched batch, every procedure in one launch
//   xdrg_rpc_gather_args   one procedure's argument bytes as a contiguous
//                          indexed stream for xdrg_decode
//
// Every call validates its arguments on the host before the first HIP call,
// launches kernels only (no memset or memcpy nodes: xdrgpu.h "Graph
// capture") and keeps no state.
#include <hip/hip_runtime.h>

#include "verify_host.h"

using namespace xdrg;
using namespace xdrg::dev;
using namespace xdrg::host;

extern "C" {

int xdrg_verify(const xdrg_plan *plan, const void *d_xdr, uint64_t xdr_len, const uint64_t *d_begin,
                const uint64_t *d_end, uint32_t span_stride, uint64_t n, uint32_t stack_limit,
                uint32_t *d_verdicts, uint64_t *d_bad_count, void *stream) {
  if (!plan || span_stride < 8u || (span_stride & 7u)) return XDRG_EINVAL;
  if (n && (!d_verdicts || !d_begin || !d_end || (!d_xdr && xdr_len))) return XDRG_EINVAL;
  if (misaligned(d_xdr, 3) || misaligned(d_begin, 7) || misaligned(d_end, 7) || misaligned(d_verdicts, 3) ||
      misaligned(d_bad_count, 7))
    return XDRG_EALIGN;
  if (n == 0) return XDRG_OK;
  const dev_tables *T = nullptr;
  const int rc = plan_tables(plan, &T);
  if (rc != XDRG_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d_bad_count) HIPCHK(static_cast<hipError_t>(fill32(d_bad_count, 0u, 2, stream)));
  const uint32_t nops = uint32_t(plan->ops.size());
  const verify_geom g = verify_geometry(plan->has_sub, size_t(nops) * sizeof(xdrg_op), n);
  if (g.nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  const uint8_t *x8 = static_cast<const uint8_t *>(d_xdr);
  auto *bad = reinterpret_cast<unsigned long long *>(d_bad_count);
  const uint64_t s8 = span_stride / 8u;
#define XDRG_VERIFY(SUB, LDSOPS)                                                                             \
  k_verify<SUB, LDSOPS><<<uint32_t(g.nb), g.nt, g.lds, s>>>(x8, xdr_len, d_begin, d_end, s8, n, T->d_ops, nops, \
                                                            T->d_table, stack_limit, d_verdicts, bad)
  if (plan->has_sub) { if (g.lds_ops) XDRG_VERIFY(true, true); else XDRG_VERIFY(true, false); }
  else { if (g.lds_ops) XDRG_VERIFY(false, true); else XDRG_VERIFY(false, false); }
#undef XDRG_VERIFY
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

int xdrg_rpc_verify_args(const void *d_stream, uint64_t len, xdrg_rpc_hdr *d_hdrs, uint64_t n,
                         const xdrg_rpc_argplan *plans, uint32_t nplans, uint32_t stack_limit,
                         uint32_t *d_verdicts, void *stream) {
  if (nplans > XDRG_RPC_MAX_ARGPLANS || (nplans && !plans)) return XDRG_EINVAL;
  for (uint32_t i = 0; i < nplans; ++i) {
    if (!plans[i].plan) return XDRG_EINVAL;
    if (i) {  // sorted by (prog, vers, proc), no duplicates
      const xdrg_rpc_argplan &x = plans[i - 1], &y = plans[i];
      const bool less = x.prog != y.prog ? x.prog < y.prog : x.vers != y.vers ? x.vers < y.vers : x.proc < y.proc;
      if (!less) return XDRG_EINVAL;
    }
  }
  if (n && (!d_hdrs || (!d_stream && len))) return XDRG_EINVAL;
  if (misaligned(d_stream, 3) || misaligned(d_hdrs, 15) || misaligned(d_verdicts, 3)) return XDRG_EALIGN;
  if (n == 0) return XDRG_OK;
  verify_argtable tab = {};
  bool sub = false;
  size_t ops_lds = 0;
  for (uint32_t i = 0; i < nplans; ++i) {
    const dev_tables *T = nullptr;
    const int rc = plan_tables(plans[i].plan, &T);
    if (rc != XDRG_OK) return rc;
    tab.e[i] = verify_argplan{T->d_ops, T->d_table, uint32_t(plans[i].plan->ops.size()), plans[i].prog,
                              plans[i].vers, plans[i].proc};
    sub = sub || plans[i].plan->has_sub;
    ops_lds += plans[i].plan->ops.size() * sizeof(xdrg_op);
  }
  const verify_geom g = verify_geometry(sub, ops_lds, n);  // every plan's ops, staged per workgroup
  if (g.nb > 0x7fffffffull) return XDRG_EUNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t *x8 = static_cast<const uint8_t *>(d_stream);
#define XDRG_VERIFY_ARGS(SUB, LDSOPS)                                                                   \
  k_rpc_verify_args<SUB, LDSOPS><<<uint32_t(g.nb), g.nt, g.lds, s>>>(x8, len, d_hdrs, n, tab, nplans, \
                                                                     stack_limit, d_verdicts)
  if (sub) { if (g.lds_ops) XDRG_VERIFY_ARGS(true, true); else XDRG_VERIFY_ARGS(true, false); }
  else { if (g.lds_ops) XDRG_VERIFY_ARGS(false, true); else XDRG_VERIFY_ARGS(false, false); }
#undef XDRG_VERIFY_ARGS
  HIPCHK(hipGetLastError());
  return XDRG_OK;
}

size_t xdrg_rpc_gather_workspace_size(uint64_t n) { return gather_ws_bytes(n); }

int xdrg_rpc_gather_args(const void *d_stream, uint64_t len, const xdrg_rpc_hdr *d_hdrs, uint64_t n,
                         uint32_t prog, uint32_t vers, uint32_t proc, uint8_t *d_args, uint64_t args_capacity,
                         uint64_t *d_offsets, uint64_t *d_index, uint64_t *d_count, void *d_workspace,
                         size_t workspace_bytes, xdrg_status *d_status, void *stream) {
  if (!d_offsets || !d_count || !d_status) return XDRG_EINVAL;
  if (n && (!d_hdrs || !d_index || (!d_stream && len))) return XDRG_EINVAL;
  if (!d_args && args_capacity) return XDRG_EINVAL;
  if (misaligned(d_hdrs, 15) || misaligned(d_offsets, 7) || misaligned(d_index, 7) || misaligned(d_count, 7) ||
      misaligned(d_workspace, 7))
    return XDRG_EALIGN;
  return launch_gather(gather_key{prog, vers, proc}, d_stream, len, d_hdrs, n, d_args, args_capacity, d_offsets,
                       d_index, d_count, d_workspace, workspace_bytes, d_status, stream);
}

}  // extern "C"
