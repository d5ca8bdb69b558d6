"""Times of xdrg_sort on 1M records of rec128 and of recvar
(W.GENERATORS), each as generated (nearly all values distinct) and with every
value repeated 8 times, each with the narrow passes in one LDS launch
(k_sort_tile) and with every pass in global memory (XDRG_SORT_TILE=0), beside
two yardsticks timed in the same run:

    torch.sort of n int64 keys    what sorting n items costs at all
    one xdrg_compare, all equal   one full walk per record: sort / compare =
                                  the walk-equivalents a sorted element costs
                                  (the rank merge predicts ~log2(n)^2 / 2
                                  probes, most of which stop early); for
                                  rec128 also from a batch that is not 16-byte
                                  aligned, which takes the walk the sort uses
                                  instead of the chunk kernel

    python tools/gpu/time_sort.py [--n 1048576] [--runs 20]

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
from time_compare import timed_flushed  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402

dev = TV.dev


def _tile(on: bool) -> None:
    os.environ["XDRG_SORT_TILE"] = "1" if on else "0"


def figures(name: str, n: int, runs: int, repeat: int) -> None:
    t = S.ALL[name]
    mar = M.Marshaler(M.Plan(t), dev)
    nat, heap = W.GENERATORS[name](n)
    st = mar.plan.stride
    rows = nat.reshape(n, st)
    lo, hi = (80, 128) if name == "rec128" else (S.recvar.offsets["score"], S.recvar.offsets["score"] + 8)
    d = rows[:, lo:hi].copy().view("<f8")  # random bit patterns hold NaNs, which are unsortable
    d[np.isnan(d)] = 0.0
    rows[:, lo:hi] = d.view(np.uint8)
    if repeat > 1:
        rows[:] = rows[np.arange(n) % (n // repeat)]
    recs = torch.from_numpy(rows.reshape(-1)).to(dev)
    dheap = torch.from_numpy(heap).to(dev) if heap.size else None
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    ws = mar.sort_workspace(n)
    keys = torch.randint(-2 ** 62, 2 ** 62, (n,), dtype=torch.int64, device=dev)
    other = recs.clone()
    oheap = dheap.clone() if dheap is not None else None
    out = torch.empty(n, dtype=torch.int8, device=dev)

    def sort(tile):
        _tile(tile)
        mar.launch_sort(recs, n, perm, first, counts, dheap, ws)

    fns = {"tile kernel": lambda: sort(True), "passes from width 1": lambda: sort(False),
           "torch.sort int64 (yardstick)": lambda: torch.sort(keys),
           "xdrg_compare all equal": lambda: mar.launch_compare(recs, other, n, out, dheap, oheap)}
    if name == "rec128":  # 8 bytes in: not the chunk kernel's
        sa = torch.empty(recs.numel() + 16, dtype=torch.uint8, device=dev)
        sb = torch.empty(recs.numel() + 16, dtype=torch.uint8, device=dev)
        sa[8:-8] = recs
        sb[8:-8] = recs
        fns["xdrg_compare all equal, walk"] = lambda: mar.launch_compare(sa[8:-8], sb[8:-8], n, out, None, None)
    tm = timed_flushed(fns, runs)
    res = {}
    for tile in (True, False):  # both variants give the same bytes
        sort(tile)
        res[tile] = (perm.clone(), first.clone(), counts.cpu().tolist())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert res[True][2] == res[False][2] and res[True][2][0] == n and not out.any().item()
    distinct = res[True][2][1]
    what = f"sort {name}" + (f" x{repeat}" if repeat > 1 else "")
    nbytes = recs.numel() + (dheap.numel() if dheap is not None else 0)
    for k, ms in tm.items():
        TV.report(f"{what}: {k}", ms, 8 * n if "torch" in k else nbytes, records=n, distinct=distinct)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    ar = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    for nm in ("rec128", "recvar"):
        for rep in (1, 8):
            figures(nm, ar.n, ar.runs, rep)
