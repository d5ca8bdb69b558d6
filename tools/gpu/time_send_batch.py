"""Times of the send batch at 1M messages:
xdrg_rpc_send_batch on the reply stream of time_reply_batch.py (every call of
time_verify.py's batch answered with its echoed arguments), routed

    (a) in connection order over 16,384 connections (the in-order fast path),
    (b) shuffled over 16,384 connections,
    (c) shuffled, one message per connection over as many connections as
        messages,
    (d) all to one connection,

beside the yardstick: what the parent of this stage offers for (a), the only
case it can express -- the reply stream is in connection order already, so
queueing it is a plain device copy of the same bytes.  The copy is timed
twice in the same alternation, so that its own spread is on the page.

    python tools/gpu/time_send_batch.py [--n 1048576] [--runs 20] [--cases abcd]

Device events in one process, after warm-up, median (and min) of --runs
runs; the figures are timed alternately.  One JSON line per figure."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_verify as TV  # noqa: E402  (call_batch, timed, report; puts the repository on sys.path)
from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402

dev = TV.dev
CONNS = 1 << 14


def reply_stream(n: int):
    """time_reply_batch.py's reply stream: (bytes, offsets int64 [n + 1], n)."""
    st, n = TV.call_batch(n)
    offs = M.index_messages(st)
    procs = torch.from_numpy(W.RPC_PROCS.view("int32").copy()).to(dev)
    hd = R.dispatch(st, offs, procs)
    sources = []
    for key, name in TV.PROCS.items():
        args, aoffs, index = R.gather_args(st, hd, key)
        fs = M.Plan(S.ALL[name]).fixed_size
        sources.append(R.ResultSource(index, args, None, fs) if fs else R.ResultSource(index, args, aoffs))
    replies, roffs = R.reply_batch(hd, sources)
    return replies, roffs, n


def main(n: int, runs: int, cases: str = "abcd") -> None:
    replies, roffs, n = reply_stream(n)
    nbytes = replies.numel()
    L = A.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(7)
    i = torch.arange(n, dtype=torch.int64)
    routes = {"a in order": (i * CONNS // n, CONNS), "b shuffled 16384": (torch.randint(0, CONNS, (n,), generator=g), CONNS),
              "c one each": (torch.randperm(n, generator=g), n), "d one connection": (torch.zeros(n, dtype=torch.int64), 1)}
    calls, state = {}, {}
    for name, (conn, nconns) in routes.items():
        if name[0] not in cases:  # a kernel trace of one case at a time
            continue
        conn = conn.to(torch.int32).to(dev)
        src = [R.SendSource(replies, roffs, conn)]
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        arrs = (torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int64, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                torch.empty(n, dtype=torch.int64, device=dev), torch.empty(4 * nconns, dtype=torch.int64, device=dev),
                torch.empty(4, dtype=torch.int64, device=dev))
        ws = torch.empty(L.xdrg_rpc_send_batch_workspace_size(n, nconns), dtype=torch.uint8, device=dev)
        status = M.Status(dev)
        state[name] = (out, arrs, status, conn, nconns)
        calls["send_batch " + name] = (lambda src=src, nconns=nconns, out=out, arrs=arrs, status=status, ws=ws:
                                       R.launch_send_batch(src, nconns, None, out, *arrs, status, ws, s))
    copy_dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fns = {"device copy (first)": lambda: copy_dst.copy_(replies)}
    fns.update(calls)
    fns["device copy (second)"] = lambda: copy_dst.copy_(replies)
    t = TV.timed(fns, runs)
    for name, (out, arrs, status, conn, nconns) in state.items():  # what was timed is what was asked for
        e = status.read(s)
        assert e.code == 0 and int(e.total_bytes) == nbytes and int(arrs[1].item()) == n, name
        assert arrs[6].tolist() == [n, 0, 0, 0], name
        order = torch.sort(conn, stable=True).indices
        assert torch.equal(arrs[3], order) and torch.equal(arrs[2], conn[order]), name
        q = R.wqueues_numpy(arrs[5])
        assert int(q["msgs"].sum()) == n and int(q["len"].sum()) == nbytes, name
        if name[0] in "ad":
            assert torch.equal(out, replies), name
        else:
            k = int(order[n // 3].item())
            a, b, at = int(roffs[k].item()), int(roffs[k + 1].item()), int(arrs[0][n // 3].item())
            assert torch.equal(out[at:at + b - a], replies[a:b]), name
    yard = statistics.median(t["device copy (first)"] + t["device copy (second)"])
    for k, ms in t.items():
        TV.report(f"send batch {k}", ms, nbytes, messages=n, ratio_to_copy=round(statistics.median(ms) / yard, 2))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--cases", default="abcd")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(a.n, a.runs, a.cases)
