"""Times of the receive batch on the 1M-call stream of
time_call_batch.py, framed as

    (a) 16,384 connections x 64 messages, every connection's tail cut at a
        seeded point inside its last message
    (b) 1M connections x 1 message
    (c) 1 connection x 1M messages

beside what a caller does today with the same bytes as one stream, which is
(c)'s buffer only: xdrg_index_msgs and a device copy of the stream.  The
yardstick is timed twice in the same alternation, for its own spread.

    python tools/gpu/time_recv_batch.py [--n 1048576] [--runs 20]

Device events in one process, after warm-up, median (and min) of --runs
runs; the figures are timed alternately.  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_verify as TV  # noqa: E402  (call_batch, timed, report; puts the repository on sys.path)
from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402

dev = TV.dev
PER = 64  # messages a connection of (a)


def figures(n: int, runs: int) -> None:
    st, n = TV.call_batch(n)
    offs = M.index_messages(st)
    o = offs.cpu().numpy().astype(np.uint64)
    total = st.numel()
    L = A.lib()
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(16)

    tables = {}
    na = n // PER
    a = np.zeros(na, dtype=A.CONN_IN_DTYPE)
    a["begin"] = o[0:na * PER:PER]
    last = o[PER:na * PER + 1:PER] - o[PER - 1:na * PER:PER]  # bytes of each connection's last message
    cut = 1 + rng.integers(0, last.astype(np.int64) - 1)  # 1 .. last - 1 bytes dropped
    a["len"] = o[PER:na * PER + 1:PER] - a["begin"] - cut.astype(np.uint64)
    tables["a"] = a
    b = np.zeros(n, dtype=A.CONN_IN_DTYPE)
    b["begin"], b["len"] = o[:-1], o[1:] - o[:-1]
    tables["b"] = b
    tables["c"] = np.array([(0, total)], dtype=A.CONN_IN_DTYPE)
    for t in tables.values():
        R.check_segs(t, total)

    max_msgs = total // 4
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    roffs = torch.empty(max_msgs + 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    cof = torch.empty(max_msgs, dtype=torch.int32, device=dev)
    kind = torch.empty(max_msgs, dtype=torch.uint8, device=dev)
    status = M.Status(dev)
    calls = {}
    for name, t in tables.items():
        d_segs = torch.from_numpy(t.view(np.int64).copy()).to(dev)
        conns = torch.empty(4 * t.size, dtype=torch.int64, device=dev)
        ws = torch.empty(L.xdrg_rpc_recv_batch_workspace_size(t.size, total), dtype=torch.uint8, device=dev)
        calls[name] = (d_segs, conns, ws)

    def recv(name):
        d_segs, conns, ws = calls[name]
        return lambda: R.launch_recv_batch(st, d_segs, A.MSG_SOCK_MAXMSGLEN, A.RECV_RPC_SOCK, out, roffs, cnt, cof,
                                           kind, conns, status, ws, s)

    # the check of what is timed
    for name, t in tables.items():
        status.init(s)
        recv(name)()
        e = status.read(s)
        k = int(cnt.item())
        c = R.conns_numpy(calls[name][1])
        assert e.code == 0 and (c["state"] == A.CONN_OPEN).all()
        if name == "a":
            assert k == na * (PER - 1) and (c["msgs"] == PER - 1).all()
            assert np.array_equal(c["need"], np.where(last.astype(np.int64) - cut >= 4, last, 4))
        else:
            assert k == n and int(e.total_bytes) == total and torch.equal(out, st) and torch.equal(roffs[:n + 1], offs)
            assert not kind[:n].any().item()  # calls

    iws = torch.empty(max(L.xdrg_index_workspace_size(total, A.MSG_SOCK_MAXMSGLEN), 16), dtype=torch.uint8, device=dev)
    ioffs = torch.empty(max_msgs + 1, dtype=torch.int64, device=dev)
    icnt = torch.empty(1, dtype=torch.int64, device=dev)
    istatus = M.Status(dev)
    copy_dst = torch.empty(total, dtype=torch.uint8, device=dev)

    def today():
        A.check(L.xdrg_index_msgs(st.data_ptr(), total, A.MSG_SOCK_MAXMSGLEN, max_msgs, ioffs.data_ptr(),
                                  icnt.data_ptr(), iws.data_ptr(), iws.numel(), istatus.ptr, s), "xdrg_index_msgs")
        copy_dst.copy_(st)

    t = TV.timed({"yardstick 1": today, "a": recv("a"), "b": recv("b"), "c": recv("c"), "yardstick 2": today}, runs)
    assert int(icnt.item()) == n and torch.equal(ioffs[:n + 1], offs)
    y1, y2 = statistics.median(t["yardstick 1"]), statistics.median(t["yardstick 2"])
    y = (y1 + y2) / 2
    # bytes: the stream in and out
    TV.report("recv_batch (a) 16,384 connections x 64 messages, tails cut", t["a"], 2 * total, connections=na,
              messages=na * (PER - 1), ratio_to_yardstick=round(statistics.median(t["a"]) / y, 3))
    TV.report("recv_batch (b) 1M connections x 1 message", t["b"], 2 * total, connections=n, messages=n,
              ratio_to_yardstick=round(statistics.median(t["b"]) / y, 3))
    TV.report("recv_batch (c) 1 connection x 1M messages", t["c"], 2 * total, connections=1, messages=n,
              ratio_to_yardstick=round(statistics.median(t["c"]) / y, 3))
    TV.report("yardstick: xdrg_index_msgs + device copy of (c)'s buffer, first", t["yardstick 1"], 2 * total, messages=n)
    TV.report("yardstick: xdrg_index_msgs + device copy of (c)'s buffer, second", t["yardstick 2"], 2 * total,
              messages=n)
    print(json.dumps({"what": "yardstick run-to-run spread (second median / first median - 1)",
                      "spread": round(y2 / y1 - 1, 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    figures(a.n, a.runs)
