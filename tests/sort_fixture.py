"""tests/golden/sort.json for the sort tests: each type's pool of 64 values
as one decoded batch (the C restatement's decode, oracle_bridge.decode) with
what the reference's std::stable_sort / std::unique recorded for it.  TEST
INFRASTRUCTURE.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import oracle_bridge as O
from compare_fixture import FLOAT_TYPES, TYPES  # noqa: F401  (re-exported)
from xdrpp_amd.xdr_types import compile_plan

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "sort.json")


@functools.lru_cache(maxsize=None)
def raw() -> dict:
    with open(PATH) as f:
        return json.load(f)["types"]


class Pool:
    """One type's pool: plan, wire bytes, the decoded batch, and the
    reference's results -- unsortable (indices with !(x == x)), sorted (the
    others by std::stable_sort), first (per sorted position: a new value)."""

    def __init__(self, name: str):
        self.name = name
        self.cp = compile_plan(TYPES[name])
        t = raw()[name]
        self.xdr = [bytes.fromhex(v) for v in t["values"]]
        self.n = len(self.xdr)
        self.unsortable = np.array(t["unsortable"], dtype=np.int64)
        self.sorted = np.array(t["sorted"], dtype=np.int64)
        self.first = np.array(t["first"], dtype=np.uint8)
        x = np.frombuffer(b"".join(self.xdr), dtype=np.uint8).copy()
        offs = np.zeros(self.n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(r) for r in self.xdr])
        self.nat, self.heap = O.decode(self.cp, x, self.n, None if self.cp.fixed_size is not None else offs)
        # what xdrg_sort gives for the pool as it stands
        self.m = len(self.sorted)
        self.perm = np.concatenate([self.sorted, self.unsortable])
        self.first_all = np.concatenate([self.first, np.ones(self.n - self.m, dtype=np.uint8)])
        self.distinct = int(self.first.sum())
        # rank[i] = the equivalence class of pool member i in ascending order (-1: unsortable)
        self.rank = np.full(self.n, -1, dtype=np.int64)
        self.rank[self.sorted] = np.cumsum(self.first) - 1
        for arr in (self.nat, self.heap, self.perm, self.first_all, self.rank):
            arr.setflags(write=False)


@functools.lru_cache(maxsize=None)
def pool(name: str) -> Pool:
    return Pool(name)


def expected_rows(p: Pool, idx: np.ndarray):
    """What xdrg_sort gives for the batch of pool rows idx (with repeats):
    (perm, first, m, distinct), from the recorded ranks alone -- a stable
    argsort of the rows' classes, the unsortable rows behind in input order."""
    rk = p.rank[idx]
    ok = np.nonzero(rk >= 0)[0]
    order = ok[np.argsort(rk[ok], kind="stable")]
    perm = np.concatenate([order, np.nonzero(rk < 0)[0]])
    srk = rk[order]
    first = np.ones(len(idx), dtype=np.uint8)
    first[1:len(order)] = srk[1:] != srk[:-1]
    return perm, first, len(order), int(first[:len(order)].sum())
