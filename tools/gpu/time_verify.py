"""Times of the per-record verdict calls at 1M records (DESIGN.md "Per-record
verdicts"): xdrg_verify on recvar and rpc beside xdrg_decode of the same
stream (the interpreter's per-lane kernel, and the default kernels), and a
1M-message call batch through dispatch, verify_args, gather_args and decode.

    python tools/gpu/time_verify.py [--n 1048576] [--runs 20]

Device events in one process, after warm-up, median (and min) of --runs
runs; the stages of a pair are timed alternately.  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402

dev = torch.device("cuda:0")


def timed(fns: dict, runs: int, warm: int = 3) -> dict:
    """{name: [ms, ...]} of each callable, run alternately (one round = each once)."""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(runs):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def report(what: str, ms: list, nbytes: int, **kw) -> None:
    med = statistics.median(ms)
    print(json.dumps({"what": what, "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "runs": len(ms),
                      "bytes": int(nbytes), "GB_per_s": round(nbytes / med / 1e6, 1), **kw}), flush=True)


def stream_schema(name: str, n: int, runs: int) -> None:
    """xdrg_verify beside xdrg_decode on one encoded stream of n records."""
    nat, heap = W.GENERATORS[name](n)
    nat, heap = torch.from_numpy(nat).to(dev), torch.from_numpy(heap).to(dev)
    enc = M.Marshaler(M.Plan(S.ALL[name]), dev).encode(nat, n, heap)
    x, offs = enc.xdr, enc.offsets
    ver = M.Marshaler(M.Plan(S.ALL[name]), dev)
    verdicts = torch.zeros(n, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    fns = {"verify": lambda: ver.launch_verify(x, offs.data_ptr(), offs.data_ptr() + 8, 8, n, verdicts, bad)}
    for label, opts in (("decode_interp_lane", {"specialize": 0, "var_decode_kernel": 1}), ("decode_default", {})):
        mar = M.Marshaler(M.Plan(S.ALL[name], opts), dev)
        native = torch.zeros(n * mar.plan.stride, dtype=torch.uint8, device=dev)
        hout = torch.zeros(max(mar.plan.decode_heap_bytes(x.numel()), 16), dtype=torch.uint8, device=dev)
        mar.status.init(torch.cuda.current_stream().cuda_stream)
        fns[label] = (lambda mar=mar, native=native, hout=hout:
                      mar.launch_decode(x, n, native, offsets=offs, heap_out=hout))
    t = timed(fns, runs)
    assert int(bad.item()) == 0 and not verdicts.any().item()
    for k, ms in t.items():
        report(f"{name} {k}", ms, x.numel(), records=n)


PROCS = {(100000, 2, 0): "rec128", (100000, 3, 1): "recvar", (100003, 3, 5): "containertest"}


def call_batch(n: int):
    """n call messages (mark + 10 header words + one record of the procedure's
    argument type), procedures in turn: a block of 65536 built on the host,
    repeated on the device."""
    blk = min(n, 1 << 16)
    keys = list(PROCS)
    recs = {}
    for k, name in PROCS.items():
        cnt = (blk + len(keys) - 1) // len(keys)
        nat, heap = W.GENERATORS[name](cnt)
        enc = M.Marshaler(M.Plan(S.ALL[name]), dev).encode(torch.from_numpy(nat).to(dev), cnt,
                                                           torch.from_numpy(heap).to(dev) if heap.size else None)
        xs = enc.xdr.cpu().numpy()
        fs = M.Plan(S.ALL[name]).fixed_size
        o = np.arange(cnt + 1) * fs if fs else enc.offsets.cpu().numpy()
        recs[k] = (xs, o)
    parts = []
    for i in range(blk):
        k = keys[i % len(keys)]
        xs, o = recs[k]
        args = xs[int(o[i // len(keys)]):int(o[i // len(keys) + 1])]
        hdr = np.array([(args.size + 40) | A.MARK_LAST, i, 0, 2, k[0], k[1], k[2], 0, 0, 0, 0], dtype=">u4")
        parts += [hdr.view(np.uint8), args]
    block = torch.from_numpy(np.concatenate(parts)).to(dev)
    return block.repeat((n + blk - 1) // blk), ((n + blk - 1) // blk) * blk


def rpc_batch(n: int, runs: int) -> None:
    st, n = call_batch(n)
    offs = M.index_messages(st)
    assert offs.numel() == n + 1
    procs = torch.from_numpy(np.ascontiguousarray(W.RPC_PROCS).view(np.int32)).to(dev)
    plans = {k: M.Plan(S.ALL[name]) for k, name in PROCS.items()}
    hd = R.dispatch(st, offs, procs)
    verdicts = R.verify_args(st, hd, plans)
    assert not verdicts.any().item()
    t = timed({"dispatch": lambda: R.dispatch(st, offs, procs),
               "verify_args": lambda: R.verify_args(st, hd, plans),
               "gather_args x3": lambda: [R.gather_args(st, hd, k) for k in plans],
               "decode_args (verify + gather + decode)": lambda: R.decode_args(st, hd, plans)}, runs)
    for k, ms in t.items():
        report(f"rpc batch {k}", ms, st.numel(), messages=n)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    for name in ("recvar", "rpc"):
        stream_schema(name, a.n, a.runs)
    rpc_batch(a.n, a.runs)
