"""Times of xdrg_compare on 1M pairs of rec128 (the chunk
kernel) and of recvar (the walk), each in two variants:

    all equal             the worst case: every byte of both sides is read
    first field differs   the walk stops at once; the chunk kernel reads all

beside a read-only pass over the same bytes in the same run (an int64 sum of
both sides' records and heaps), the yardstick: the parent has no device path
to compare against.  tools/probe/copy_ceiling gives the box's copy number.

    python tools/gpu/time_compare.py [--n 1048576] [--runs 20]

Device events in one process, after warm-up, median (and min) of --runs
runs, the figures timed alternately, a 512 MiB buffer rewritten before every
timed launch so that no run starts with its operands in the cache.  One JSON
line per figure."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_verify as TV  # noqa: E402  (report; puts the repository on sys.path)
from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402

dev = TV.dev


def timed_flushed(fns: dict, runs: int, warm: int = 3) -> dict:
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for i in range(runs):
        for k, f in fns.items():
            flush.fill_(i & 0xff)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def _words(t):
    return t[:t.numel() // 8 * 8].view(torch.int64)


def figures(name: str, n: int, runs: int) -> None:
    t = S.ALL[name]
    mar = M.Marshaler(M.Plan(t), dev)
    nat, heap = W.GENERATORS[name](n)
    st = mar.plan.stride
    rows = nat.reshape(n, st)
    if name == "rec128":  # random bit patterns hold NaNs, which are unordered against themselves
        d = rows[:, 80:128].copy().view("<f8")
        d[np.isnan(d)] = 0.0
        rows[:, 80:128] = d.view(np.uint8)
    else:
        sc = rows[:, S.recvar.offsets["score"]:][:, :8].copy().view("<f8")
        sc[np.isnan(sc)] = 0.0
        rows[:, S.recvar.offsets["score"]:][:, :8] = sc.view(np.uint8)
    a = torch.from_numpy(nat).to(dev)
    ha = torch.from_numpy(heap).to(dev) if heap.size else None
    b_eq = a.clone()
    hb = ha.clone() if ha is not None else None
    first = rows.copy()
    first[:, 0] ^= 1  # rec128.a0 / recvar.id: the first field
    b_first = torch.from_numpy(first.reshape(-1)).to(dev)
    out_eq = torch.empty(n, dtype=torch.int8, device=dev)
    out_first = torch.empty(n, dtype=torch.int8, device=dev)
    sink = torch.empty(4, dtype=torch.int64, device=dev)

    def read_pass():
        sink[0] = _words(a).sum()
        sink[1] = _words(b_eq).sum()
        if ha is not None:
            sink[2] = _words(ha).sum()
            sink[3] = _words(hb).sum()

    tm = timed_flushed({
        "all equal": lambda: mar.launch_compare(a, b_eq, n, out_eq, ha, hb),
        "first field differs": lambda: mar.launch_compare(a, b_first, n, out_first, ha, hb),
        "read-only pass (yardstick)": read_pass}, runs)
    assert not out_eq.any().item() and (out_first != A.CMP_EQUAL).all().item()
    nbytes = 2 * a.numel() + (2 * ha.numel() if ha is not None else 0)
    touched = nbytes if mar.plan.is_fixed else 2 * 16 * n  # the walk stops after the first field's line
    TV.report(f"compare {name} all equal", tm["all equal"], nbytes, pairs=n)
    TV.report(f"compare {name} first field differs", tm["first field differs"], touched, pairs=n)
    TV.report(f"compare {name} read-only pass over the same bytes (yardstick)", tm["read-only pass (yardstick)"],
              nbytes, pairs=n)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    ar = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    for nm in ("rec128", "recvar"):
        figures(nm, ar.n, ar.runs)
