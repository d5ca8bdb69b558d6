"""Times of settling a reply batch on the table DESIGN.md
7.2.4 measured: 1M new calls on 262,144 pending ones, about 1.3M entries, half
of them answered.

    xdrg_rpc_pending_retire            the table after the erases
    xdrg_rpc_call_stats                every call's rpc_call_stat, n = 1M headers
    xdrg_rpc_pending_add               the yardstick: producing a table of the
                                       same length (it searches per entry)
    device copy                        the ceiling: the table's bytes, copied
    numpy mask + upload (wall clock)   the host alternative: the table
                                       downloaded, a boolean mask, the upload

    python tools/gpu/time_settle.py [--n 1048576] [--runs 20]

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
import time_verify as TV  # noqa: E402  (timed, report; puts the repository on sys.path)
from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402

dev = TV.dev
OLD = 1 << 18  # calls pending before the batch


def figures(n: int, runs: int) -> None:
    rng = np.random.default_rng(3)
    last = 0xFFF00000  # the new xids wrap
    near = (last + 1 + rng.integers(0, 2 * n, size=OLD // 2)) & 0xFFFFFFFF
    far = rng.integers(0x1000000, 0xF0000000, size=OLD)
    old = rng.permutation(np.unique(np.concatenate([near, far]).astype(np.uint32)))[:OLD]
    p0 = R.PendingCalls(old, (np.arange(old.size) % 3).astype(np.uint32), dev, last_xid=last)
    s = torch.cuda.current_stream().cuda_stream
    xids = torch.empty(n, dtype=torch.int32, device=dev)
    new = torch.empty(n, dtype=torch.int64, device=dev)
    nc = p0.ncalls + n
    merged = torch.empty(nc, dtype=torch.int64, device=dev)
    pos = torch.empty(nc, dtype=torch.int64, device=dev)
    R.launch_next_xids(p0, xids, s)
    new.copy_((xids.to(torch.int64) & 0xFFFFFFFF) | (1 << 32))  # res = 1
    R.launch_pending_add(p0, new, merged, pos[:p0.ncalls], pos[p0.ncalls:], s)
    p = R.PendingCalls.from_device(merged.clone(), torch.arange(nc, dtype=torch.int64, device=dev), last_xid=last)

    # half of the table answered, by n messages in a shuffled order; the headers every reply kind in turn
    answered = rng.random(nc) < 0.5
    reply_of_h = np.full(nc, -1, dtype=np.int64)
    reply_of_h[answered] = rng.integers(n, size=int(answered.sum()))
    reply_of = torch.from_numpy(reply_of_h).to(dev)
    hdrs_h = np.zeros(n, dtype=R.HDR_DTYPE)
    hdrs_h["action"] = np.arange(n) % 4
    hdrs_h["w"][:, A.RPC_W_STAT], hdrs_h["w"][:, A.RPC_W_WHY] = 4, 5
    hdrs = torch.from_numpy(hdrs_h.view(np.uint8).reshape(-1)).to(dev)

    stats = torch.empty(nc, dtype=torch.int64, device=dev)
    kept = torch.empty(nc, dtype=torch.int64, device=dev)
    kept_pos = torch.empty(nc, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(A.lib().xdrg_rpc_pending_retire_workspace_size(nc), 16), dtype=torch.uint8, device=dev)
    merged2 = torch.empty(nc, dtype=torch.int64, device=dev)
    copy_dst = torch.empty(nc, dtype=torch.int64, device=dev)
    t = TV.timed({
        "pending_retire": lambda: R.launch_pending_retire(p, reply_of, kept, kept_pos, count, ws, s),
        "call_stats": lambda: R.launch_call_stats(hdrs, reply_of, stats, A.RPCS_PENDING, s),
        "pending_add (yardstick)": lambda: R.launch_pending_add(p0, new, merged2, pos[:p0.ncalls], pos[p0.ncalls:], s),
        "device copy (ceiling)": lambda: copy_dst.copy_(p.table)}, runs)

    # the host alternative, and the check of what was timed
    table_h = None
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table_h = p.table.cpu().numpy()
        mask = reply_of.cpu().numpy() == -1
        up = torch.from_numpy(table_h[mask]).to(dev)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    k = int(count.item())
    assert k == int((~answered).sum()) and torch.equal(kept[:k], up) and torch.equal(merged2, merged)
    want_pos = np.where(~answered, np.cumsum(~answered) - 1, -1)
    assert np.array_equal(kept_pos.cpu().numpy(), want_pos)
    got = R.call_stats_numpy(stats)
    assert (got["type"][~answered] == A.RPCS_PENDING).all() and (got["type"][answered] != A.RPCS_PENDING).all()

    # bytes: reply_of twice, the kept entries in and out, kept_pos | reply_of, a header line per answered call,
    # the stats | the entries in, the table and the positions out (the searches not counted) | in and out
    TV.report("settle pending_retire", t["pending_retire"], 24 * nc + 16 * k, entries=nc, kept=k)
    TV.report("settle call_stats", t["call_stats"], 16 * nc + 64 * int(answered.sum()), entries=nc, headers=n)
    TV.report("settle pending_add (yardstick: a table of the same length)", t["pending_add (yardstick)"], 24 * nc,
              entries=nc, pending_before=p0.ncalls)
    TV.report("settle device copy of the table (ceiling)", t["device copy (ceiling)"], 16 * nc, entries=nc)
    print(json.dumps({"what": "settle numpy mask over the downloaded table + upload (wall clock)",
                      "median_ms": round(statistics.median(wall), 3), "min_ms": round(min(wall), 3),
                      "runs": len(wall), "entries": nc, "kept": k}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    figures(a.n, a.runs)
