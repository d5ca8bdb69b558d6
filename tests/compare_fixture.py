"""tests/golden/compare.json for the comparison tests: the types of the
fixture as xdrc-mirror descriptors, and each type's pairs as two decoded
batches (the C restatement's decode, oracle_bridge.decode) with the
reference's recorded results.  TEST INFRASTRUCTURE.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import oracle_bridge as O
from xdrpp_amd import schemas as S
from xdrpp_amd.xdr_types import (Bool, Double, Enum, Int, Pointer, String, UInt, Union, Void, compile_plan)

HERE = os.path.dirname(os.path.abspath(__file__))

# tests/xdrtest.x:18-27, :58-69, :139-144
uunion = Union("uunion", "d", UInt, [([1], "one", Bool), ([2], "two", Int), ([3], "three", Double),
                                     ([4], "four", String())])
# a bool discriminant decodes true from any nonzero word (types.h:335-349), so TRUE is every value but 0
uptr = Union("uptr", "b", Bool, [([0], "", Void)], default=("val", Pointer(Int)))
color = Enum("color", {"RED": 0, "REDDER": 1, "REDDEST": 2})
ContainsEnum = Union("ContainsEnum", "c", color, [([0], "foo", String()),
                                                  ([1], "num", Enum("_num_t", {"ONE": 0, "TWO": 1}))])

TYPES = {"numerics": S.numerics, "rec128": S.rec128, "recvar": S.recvar, "rpc_msg": S.rpc_msg, "uunion": uunion,
         "uptr": uptr, "ContainsEnum": ContainsEnum, "containertest": S.containertest, "hasbytes": S.hasbytes,
         "test_recursive": S.test_recursive, "rp__list": S.rp__list}
FLOAT_TYPES = ("numerics", "rec128", "recvar", "uunion", "containertest")


@functools.lru_cache(maxsize=None)
def raw() -> dict:
    with open(os.path.join(HERE, "golden", "compare.json")) as f:
        return json.load(f)["types"]


def _side_b(a: bytes, b: str) -> bytes:
    """b's wire bytes: "" = a again, "@pos=xx" = a with byte pos set to xx, else hex."""
    if not b:
        return a
    if b[0] == "@":
        pos, val = b[1:].split("=")
        return a[:int(pos)] + bytes([int(val, 16)]) + a[int(pos) + 1:]
    return bytes.fromhex(b)


class Batch:
    """One type's pairs: plan, both sides' wire bytes and decoded batches,
    the reference's a <=> b (cmp) and a == b (eq)."""

    def __init__(self, name: str):
        self.name = name
        self.cp = compile_plan(TYPES[name])
        pairs = raw()[name]["pairs"]
        self.n = len(pairs)
        self.how = [p[0] for p in pairs]  # rows: [how, a, b, cmp, eq]
        self.xdr_a = [bytes.fromhex(p[1]) for p in pairs]
        self.xdr_b = [_side_b(a, p[2]) for a, p in zip(self.xdr_a, pairs)]
        self.cmp = np.array([p[3] for p in pairs], dtype=np.int8)
        self.eq = np.array([bool(p[4]) for p in pairs])
        self.nat_a, self.heap_a = self._decode(self.xdr_a)
        self.nat_b, self.heap_b = self._decode(self.xdr_b)
        for arr in (self.nat_a, self.heap_a, self.nat_b, self.heap_b):
            arr.setflags(write=False)

    def _decode(self, recs):
        x = np.frombuffer(b"".join(recs), dtype=np.uint8).copy()
        offs = np.zeros(len(recs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(r) for r in recs])
        return O.decode(self.cp, x, len(recs), None if self.cp.fixed_size is not None else offs)


@functools.lru_cache(maxsize=None)
def batch(name: str) -> Batch:
    return Batch(name)
