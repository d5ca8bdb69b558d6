"""Times of the asynchronous client's reply step at 1M replies (DESIGN.md
§7.2.2): check_replies, the join (xdrg_rpc_match_replies), verify_results,
gather_results per result type and decode_results, on success replies of
three result types in turn (rec128, recvar, containertest) with a 1M-entry
pending table and 1 % replies to unknown xids; and, on a call batch of the
same size, the siblings they stand beside: xdrg_rpc_dispatch and verify_args.

    python tools/gpu/time_replies.py [--n 1048576] [--runs 20]

Device events in one process, after warm-up, median (and min) of --runs
runs; the stages are timed alternately.  One JSON line per figure."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_verify as TV  # noqa: E402  (timed, report, call_batch; puts the package on sys.path)
from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402

dev = TV.dev
RES = {0: "rec128", 1: "recvar", 2: "containertest"}


def xid_of(i: np.ndarray) -> np.ndarray:
    """A bijection of the 32-bit words: distinct i give distinct xids."""
    return (i.astype(np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)


def reply_batch(n: int):
    """n success replies (mark + rpc_success_hdr + one record of the result
    type), types in turn: a block of 65536 built on the host, repeated on the
    device, then every message's xid written in place.  Message i answers
    call i, except every 100th, whose xid is in no table."""
    blk = min(n, 1 << 16)
    recs = {}
    for r, name in RES.items():
        cnt = (blk + len(RES) - 1) // len(RES)
        nat, heap = W.GENERATORS[name](cnt)
        plan = M.Plan(S.ALL[name])
        enc = M.Marshaler(plan, dev).encode(torch.from_numpy(nat).to(dev), cnt,
                                            torch.from_numpy(heap).to(dev) if heap.size else None)
        fs = plan.fixed_size
        recs[r] = (enc.xdr.cpu().numpy(), np.arange(cnt + 1) * fs if fs else enc.offsets.cpu().numpy())
    parts = []
    for i in range(blk):
        xs, o = recs[i % len(RES)]
        res = xs[int(o[i // len(RES)]):int(o[i // len(RES) + 1])]
        parts += [np.array([(res.size + 24) | A.MARK_LAST, 0, 1, 0, 0, 0, 0], dtype=">u4").view(np.uint8), res]
    reps = (n + blk - 1) // blk
    n = reps * blk
    st = torch.from_numpy(np.concatenate(parts)).to(dev).repeat(reps)
    offs = M.index_messages(st)
    assert offs.numel() == n + 1
    i = np.arange(n, dtype=np.uint64)
    table_xids = xid_of(i)
    sent = xid_of(np.where(i % 100 == 99, i + n, i))
    st.view(torch.int32)[(offs[:-1] + 4) // 4] = torch.from_numpy(sent.byteswap().view(np.int32)).to(dev)
    pending = R.PendingCalls(table_xids, (i % blk % len(RES)).astype(np.uint32), dev)  # the block repeats
    return st, offs, pending, n


def replies(n: int, runs: int) -> None:
    st, offs, pending, n = reply_batch(n)
    plans = {r: M.Plan(S.ALL[name]) for r, name in RES.items()}
    hd, call, reply_of = R.match_replies(st, offs, pending)
    tcall = pending.to_table(call)
    treply = torch.empty(pending.ncalls, dtype=torch.int64, device=dev)
    v = R.verify_results(st, hd, call, pending, plans)
    h = R.hdrs_numpy(hd)
    assert not v.any().item(), "a result does not verify"
    assert int((reply_of < 0).sum().item()) == n // 100
    assert np.count_nonzero(h["action"] == A.RPCR_UNKNOWN_XID) == n // 100
    verdicts = torch.zeros(n, dtype=torch.int32, device=dev)
    plan_list = [plans[r] for r in sorted(plans)]
    t = TV.timed({
        "check_replies": lambda: R.check_replies(st, offs),
        "match (xdrg_rpc_match_replies)": lambda: R.launch_match_replies(st, offs, pending, hd, tcall, treply),
        "match_replies (check + match + caller's positions)": lambda: R.match_replies(st, offs, pending),
        "verify_results (xdrg_rpc_verify_results)": lambda: R.launch_verify_results(
            st, hd, tcall, pending, plan_list, 0, A.DEFAULT_STACK_LIMIT, verdicts),
        "gather_results x3": lambda: [R.gather_results(st, hd, call, pending, r) for r in plans],
        "decode_results (check + match + verify + gather + decode)": lambda: R.decode_results(st, offs, pending, plans),
    }, runs)
    for k, ms in t.items():
        TV.report(f"reply batch {k}", ms, st.numel(), messages=n, pending=pending.ncalls)


def calls(n: int, runs: int) -> None:
    st, n = TV.call_batch(n)
    offs = M.index_messages(st)
    procs = torch.from_numpy(np.ascontiguousarray(W.RPC_PROCS).view(np.int32)).to(dev)
    plans = {k: M.Plan(S.ALL[name]) for k, name in TV.PROCS.items()}
    hd = R.dispatch(st, offs, procs)
    assert not R.verify_args(st, hd, plans).any().item()
    t = TV.timed({"dispatch": lambda: R.dispatch(st, offs, procs),
                  "verify_args": lambda: R.verify_args(st, hd, plans)}, runs)
    for k, ms in t.items():
        TV.report(f"call batch {k}", ms, st.numel(), messages=n)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    replies(a.n, a.runs)
    calls(a.n, a.runs)
