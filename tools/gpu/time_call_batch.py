"""Times of the client's call stream at 1M calls:
xdrg_rpc_call_batch on the call batch of time_verify.py (rec128, recvar and
containertest procedures in turn), its argument sources the three
xdrg_rpc_gather_args of that batch's stream, beside its yardsticks:
xdrg_rpc_reply_batch on the same sources (the sibling: 28-byte headers where
the call stream has 44) and a plain device copy of the same number of output
bytes (the ceiling).  Then the pending table: xdrg_rpc_next_xids +
xdrg_rpc_pending_add on the device beside the host PendingCalls constructor
on the same xids (wall clock, its upload included).

    python tools/gpu/time_call_batch.py [--n 1048576] [--runs 20]

Device events in one process, after warm-up, median (and min) of --runs
runs; the figures are timed alternately.  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_verify as TV  # noqa: E402  (call_batch, timed, report; puts the repository on sys.path)
from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402

dev = TV.dev
OLD = 1 << 18  # calls pending before the batch


def stream_figures(n: int, runs: int) -> None:
    st, n = TV.call_batch(n)
    offs = M.index_messages(st)
    procs = torch.from_numpy(W.RPC_PROCS.view("int32").copy()).to(dev)
    hd = R.dispatch(st, offs, procs)
    L = A.lib()
    s = torch.cuda.current_stream().cuda_stream
    args_srcs, res_srcs = [], []
    for p, (key, name) in enumerate(TV.PROCS.items()):
        args, aoffs, index = R.gather_args(st, hd, key)
        fs = M.Plan(S.ALL[name]).fixed_size
        args_srcs.append(R.ArgSource(key, p, index, args, None, fs) if fs else R.ArgSource(key, p, index, args, aoffs))
        res_srcs.append(R.ResultSource(index, args, None, fs) if fs else R.ResultSource(index, args, aoffs))
    arg_bytes = sum(r.xdr.numel() for r in args_srcs)
    # the xids of time_verify's stream, so that the output must be that stream
    blk = min(n, 1 << 16)
    xids = (torch.arange(n, dtype=torch.int64, device=dev) % blk).to(torch.int32)

    cap = 44 * n + arg_bytes
    assert cap == st.numel()
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    coffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sent = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(L.xdrg_rpc_call_batch_workspace_size(n), dtype=torch.uint8, device=dev)
    status = M.Status(dev)

    rcap = 28 * n + arg_bytes
    rout = torch.empty(rcap, dtype=torch.uint8, device=dev)
    roffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    unused = torch.zeros(1, dtype=torch.int64, device=dev)
    rws = torch.empty(L.xdrg_rpc_reply_batch_workspace_size(n), dtype=torch.uint8, device=dev)
    rstatus = M.Status(dev)

    copy_dst = torch.empty(cap, dtype=torch.uint8, device=dev)
    t = TV.timed({"call_batch": lambda: R.launch_call_batch(xids, args_srcs, out, coffs, sent, counts, status, ws, s),
                  "reply_batch (28-byte headers)": lambda: R.launch_reply_batch(hd, res_srcs, rout, roffs, unused,
                                                                                 rstatus, rws, s),
                  "device copy": lambda: copy_dst.copy_(out)}, runs)
    e = status.read(s)
    assert e.code == 0 and int(e.total_bytes) == cap and counts.cpu().tolist() == [0, 0]
    assert torch.equal(out, st) and torch.equal(coffs, offs)  # the stream the sources were gathered from
    assert rstatus.read(s).code == 0 and int(unused.item()) == 0
    for k, ms in t.items():
        TV.report(f"call stream {k}", ms, rcap if k.startswith("reply") else cap, messages=n)


def pending_figures(n: int, runs: int) -> None:
    rng = np.random.default_rng(3)
    last = 0xFFF00000  # the new xids wrap
    near = (last + 1 + rng.integers(0, 2 * n, size=OLD // 2)) & 0xFFFFFFFF
    far = rng.integers(0x1000000, 0xF0000000, size=OLD)
    old = rng.permutation(np.unique(np.concatenate([near, far]).astype(np.uint32)))[:OLD]
    old_res = (np.arange(old.size) % 3).astype(np.uint32)
    p = R.PendingCalls(old, old_res, dev, last_xid=last)
    s = torch.cuda.current_stream().cuda_stream
    xids = torch.empty(n, dtype=torch.int32, device=dev)
    new = torch.empty(n, dtype=torch.int64, device=dev)
    merged = torch.empty(p.ncalls + n, dtype=torch.int64, device=dev)
    pos = torch.empty(p.ncalls + n, dtype=torch.int64, device=dev)
    R.launch_next_xids(p, xids, s)
    new.copy_((xids.to(torch.int64) & 0xFFFFFFFF) | (1 << 32))  # res = 1

    def device():
        R.launch_next_xids(p, xids, s)
        R.launch_pending_add(p, new, merged, pos[:p.ncalls], pos[p.ncalls:], s)

    t = TV.timed({"next_xids + pending_add": device}, runs)
    hx = np.concatenate([old, xids.cpu().numpy().view(np.uint32)])
    hr = np.concatenate([old_res, np.ones(n, dtype=np.uint32)])
    wall = []
    for _ in range(max(3, runs // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q = R.PendingCalls(hx, hr, dev)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(merged, q.table) and torch.equal(torch.cat([pos[:p.ncalls][p.inv], pos[p.ncalls:]]), q.inv)
    TV.report("pending table next_xids + pending_add (device)", t["next_xids + pending_add"], 8 * (p.ncalls + n),
              calls=n, pending_before=p.ncalls)
    print(json.dumps({"what": "pending table PendingCalls(...) on the host, upload included (wall clock)",
                      "median_ms": round(statistics.median(wall), 3), "min_ms": round(min(wall), 3),
                      "runs": len(wall), "calls": n, "pending_before": p.ncalls}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    stream_figures(a.n, a.runs)
    pending_figures(a.n, a.runs)
