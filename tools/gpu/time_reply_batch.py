"""Times of the server's reply stream at 1M messages:
xdrg_rpc_reply_batch on the call batch of time_verify.py (rec128, recvar and
containertest procedures in turn) with the echoed arguments as results, at
both copy widths of its emit kernel (16 bytes a lane, the default, and 4 with
XDRG_REPLY_BATCH_COPY=4), beside the two yardsticks: the three
xdrg_rpc_gather_args launches on the same batch (the same bytes the other
way) and a plain device copy of the same number of output bytes (the
ceiling).

    python tools/gpu/time_reply_batch.py [--n 1048576] [--runs 20]

Device events in one process, after warm-up, median (and min) of --runs
runs; the figures are timed alternately.  One JSON line per figure."""
import argparse
import os
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
ENV = "XDRG_REPLY_BATCH_COPY"


def main(n: int, runs: int) -> None:
    st, n = TV.call_batch(n)
    offs = M.index_messages(st)
    procs = torch.from_numpy(W.RPC_PROCS.view("int32").copy()).to(dev)
    hd = R.dispatch(st, offs, procs)
    L = A.lib()
    s = torch.cuda.current_stream().cuda_stream
    # the handlers echo: each procedure's gathered arguments are its results
    sources, gathers = [], []
    for key, name in TV.PROCS.items():
        args, aoffs, index = R.gather_args(st, hd, key)
        fs = M.Plan(S.ALL[name]).fixed_size
        sources.append(R.ResultSource(index, args, None, fs) if fs else R.ResultSource(index, args, aoffs))
        gathers.append((key, torch.empty_like(args), torch.empty(n + 1, dtype=torch.int64, device=dev),
                        torch.empty(n, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)))
    gws = torch.empty(max(L.xdrg_rpc_gather_workspace_size(n), 16), dtype=torch.uint8, device=dev)
    gst = M.Status(dev)

    def gather3():
        for (prog, vers, proc), out, o, idx, cnt in gathers:
            A.check(L.xdrg_rpc_gather_args(st.data_ptr(), st.numel(), hd.data_ptr(), n, prog, vers, proc,
                                           out.data_ptr(), out.numel(), o.data_ptr(), idx.data_ptr(), cnt.data_ptr(),
                                           gws.data_ptr(), gws.numel(), gst.ptr, s), "xdrg_rpc_gather_args")

    result_bytes = sum(r.xdr.numel() for r in sources)
    cap = 28 * n + result_bytes
    outs = {w: torch.empty(cap, dtype=torch.uint8, device=dev) for w in (16, 4)}
    roffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    unused = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.xdrg_rpc_reply_batch_workspace_size(n), dtype=torch.uint8, device=dev)
    status = M.Status(dev)

    def reply(width: int):
        if width == 4:
            os.environ[ENV] = "4"
        else:
            os.environ.pop(ENV, None)
        R.launch_reply_batch(hd, sources, outs[width], roffs, unused, status, ws, s)

    copy_dst = torch.empty(cap, dtype=torch.uint8, device=dev)
    t = TV.timed({"reply_batch copy16": lambda: reply(16), "reply_batch copy4": lambda: reply(4),
                  "gather_args x3": gather3, "device copy": lambda: copy_dst.copy_(outs[16])}, runs)
    os.environ.pop(ENV, None)
    e = status.read(s)
    assert e.code == 0 and int(e.total_bytes) == cap and int(unused.item()) == 0
    assert torch.equal(outs[16], outs[4])
    chk = R.hdrs_numpy(R.check_replies(outs[16], roffs))  # every call is answered with a success reply
    assert (chk["action"] == A.RPCR_OK).all() and gst.read(s).code == 0
    for k, ms in t.items():
        TV.report(f"reply stream {k}", ms, result_bytes if k.startswith("gather") else cap, messages=n)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    main(a.n, a.runs)
