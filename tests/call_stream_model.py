"""numpy model of the client call batch (include/xdrgpu.h "Client call
batch"), restated from the contract:

    next_xids()    rpc_sock::get_xid (xdrpp/msgsock.h:118-122) as a literal
                   loop over a set, each xid sent before the next is taken
    model()        the call stream of xdrg_rpc_call_batch, d_sent, d_counts
    merge()        calls_ after the sends: np.argsort

GoldenBatch is the batch both test files use: 1024 calls to the 61 registered
procedures of workloads.RPC_PROCS, their arguments the reference's encoded
rec128 / recvar records.  XID_CASES are the pending tables the xid and merge
tests run on.
"""
import os
from typing import NamedTuple

import numpy as np

from conftest import GOLD

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
from xdrpp_amd import workloads as W

MAX_MSG = A.MAX_MSG
UNSENT = A.RPC_RES_UNSENT
M32 = 0xFFFFFFFF


def g(name, dtype=np.uint8):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


# ------------------------------------------------------------------ xids
def next_xids(pending, last: int, n: int) -> np.ndarray:
    """get_xid() n times, each followed by send_call.  One departure from the
    reference, as in the header: a pending 0 is skipped like any other xid."""
    calls = set(int(x) for x in pending)
    assert len(calls) + n <= M32
    out, xid = [], last & M32
    for _ in range(n):
        xid = (xid + 1) & M32
        while xid in calls:
            xid = (xid + 1) & M32
        calls.add(xid)
        out.append(xid)
    return np.array(out, dtype=np.uint32)


def next_xids_by_search(pending, last: int, n: int) -> np.ndarray:
    """The formula the kernel uses, lane by lane: rotated coordinates, the
    table split at lower_bound(last + 1), the smallest j with R[j] - j > k."""
    t = np.sort(np.asarray(pending, dtype=np.uint32))
    base = (last + 1) & M32
    s = int(np.searchsorted(t, np.uint32(base), side="left"))
    rot = ((np.concatenate([t[s:], t[:s]]).astype(np.int64) - base) & M32)
    assert (np.diff(rot) > 0).all()
    key = rot - np.arange(rot.size)  # non-decreasing
    out = []
    for k in range(n):
        j = int(np.searchsorted(key, k, side="right"))
        out.append((base + k + j) & M32)
    return np.array(out, dtype=np.uint32)


def merge(old_xids, old_res, new_xids, new_res):
    """(table CALL_DTYPE [ncalls + n], old_pos, new_pos): the sorted old
    table and the new entries, sorted together."""
    x = np.concatenate([np.asarray(old_xids, dtype=np.uint32), np.asarray(new_xids, dtype=np.uint32)])
    r = np.concatenate([np.asarray(old_res, dtype=np.uint32), np.asarray(new_res, dtype=np.uint32)])
    order = np.argsort(x, kind="stable")
    t = np.empty(x.size, dtype=R.CALL_DTYPE)
    t["xid"], t["res"] = x[order], r[order]
    pos = np.empty(x.size, dtype=np.uint64)
    pos[order] = np.arange(x.size, dtype=np.uint64)
    return t, pos[:len(old_xids)], pos[len(old_xids):]


def merge_by_search(old_xids, new_xids):
    """(old_pos, new_pos) by the kernel's placement: the wrap point by a
    search, lower bounds, ranks."""
    t = np.asarray(old_xids, dtype=np.uint32)
    x = np.asarray(new_xids, dtype=np.uint32)
    n = x.size
    w = n if n == 0 else int(np.nonzero(np.append(x < x[0], True))[0][0])
    before, after = x[:w], x[w:]
    old_pos = [j + int(np.searchsorted(before, v)) + int(np.searchsorted(after, v)) for j, v in enumerate(t)]
    new_pos = [int(np.searchsorted(t, v)) + ((n - w) + k if k < w else k - w) for k, v in enumerate(x)]
    return np.array(old_pos, dtype=np.uint64), np.array(new_pos, dtype=np.uint64)


def _run(start: int, count: int) -> np.ndarray:
    return ((start + np.arange(count, dtype=np.int64)) & M32).astype(np.uint32)


def _xid_cases():
    rng = np.random.default_rng(41)
    far = np.unique(rng.integers(0x10000000, 0xE0000000, size=40, dtype=np.int64)).astype(np.uint32)
    cases = [("empty", np.zeros(0, np.uint32), 0, 5),
             ("empty_wrap", np.zeros(0, np.uint32), 0xFFFFFFFE, 257),
             ("pending_zero", np.array([0xFFFFFFFF, 0, 2], dtype=np.uint32), 0xFFFFFFFD, 8)]
    for length in (1, 63, 64, 65, 1000):
        last = 0x1000 + length
        cases.append((f"run{length}", np.concatenate([_run(last + 1, length), far]), last, 70))
    cases.append(("run64_n1", np.concatenate([_run(0x501, 64), far]), 0x500, 1))
    cases.append(("straddle", np.concatenate([_run(0xFFFFFFFF - 99, 300), far]), 0xFFFFFF00, 257))
    # gaps between short runs, the last pending value exactly at the end of the new range
    scattered = np.unique(np.concatenate([_run(0x7000 + 3 * k, 2) for k in range(0, 90, 2)] + [far]))
    cases.append(("scattered", scattered, 0x6FFF, 257))
    cases.append(("last_is_max", np.concatenate([_run(0, 3), far]), 0xFFFFFFFF, 65))
    return cases


XID_CASES = _xid_cases()  # (name, pending xids, last_xid, n)


# ---------------------------------------------------------------- stream
class Src(NamedTuple):
    """One xdrg_rpc_arg_src on the host.  count: what *d_count holds (None:
    no d_count); len(index) is count_cap.  bytes_len: None = len(xdr)."""
    key: tuple
    res: int
    index: np.ndarray                  # uint64 call positions
    xdr: np.ndarray | None = None      # None: no arguments
    offsets: np.ndarray | None = None  # None: fixed_size
    fixed_size: int = 0
    count: int | None = None
    bytes_len: int | None = None

    @property
    def entries(self) -> int:
        cap = len(self.index)
        return cap if self.count is None else min(int(self.count), cap)

    def span(self, k: int) -> tuple[int, int]:
        if self.xdr is None:
            return 0, 0
        if self.offsets is None:
            return k * self.fixed_size, (k + 1) * self.fixed_size
        return int(self.offsets[k]), int(self.offsets[k + 1])

    @property
    def length(self) -> int:
        if self.xdr is None:
            return 0
        return int(self.xdr.size) if self.bytes_len is None else self.bytes_len


def call_header(xid: int, key, L: int) -> np.ndarray:
    """The mark and rpc_msg's ten words for a call (arpc.h:44-48)."""
    prog, vers, proc = key
    return np.array([(40 + L) | A.MARK_LAST, xid, 0, 2, prog, vers, proc, 0, 0, 0, 0], dtype=">u4").view(np.uint8)


def usable(n: int, s: Src, k: int) -> bool:
    if int(s.index[k]) >= n:
        return False
    a, b = s.span(k)
    if b < a or b > s.length or a % 4 or (b - a) % 4:
        return False
    return 40 + (b - a) <= MAX_MSG


def owners(n: int, sources: list) -> tuple[dict, int]:
    """{position: (source, entry)} of the winning entries, and the entries."""
    own, entries = {}, 0
    for si, s in enumerate(sources):  # ascending (source, position): the first claim is the lowest
        for k in range(s.entries):
            entries += 1
            if usable(n, s, k):
                own.setdefault(int(s.index[k]), (si, k))
    return own, entries


def model(xids, sources: list, capacity: int | None = None):
    """(stream, offsets uint64 [n + 1], sent CALL_DTYPE [n], counts (unsent,
    unused), err): err is None or (XDRG_ERR_OVERFLOW_PUT, position); with an
    error the stream holds the messages before that position."""
    xids = np.asarray(xids, dtype=np.uint32)
    n = len(xids)
    own, entries = owners(n, sources)
    msgs = []
    sent = np.zeros(n, dtype=R.CALL_DTYPE)
    sent["xid"], sent["res"] = xids, UNSENT
    for i in range(n):
        if i not in own:
            msgs.append(np.zeros(0, np.uint8))
            continue
        si, k = own[i]
        s = sources[si]
        a, b = s.span(k)
        body = s.xdr[a:b] if b > a else np.zeros(0, np.uint8)
        msgs.append(np.concatenate([call_header(int(xids[i]), s.key, b - a), body]))
        sent["res"][i] = s.res
    offsets = np.concatenate([[0], np.cumsum([m.size for m in msgs])]).astype(np.uint64)
    err, upto = None, n
    if capacity is not None:
        bad = [i for i in range(n) if msgs[i].size and int(offsets[i + 1]) > capacity]
        if bad:
            err, upto = (A.ERR_OVERFLOW_PUT, bad[0]), bad[0]
    stream = np.concatenate(msgs[:upto] + [np.zeros(0, np.uint8)])
    return stream, offsets, sent, (n - len(own), entries - len(own)), err


# --------------------------------------------------------- the golden batch
REC128, RECVAR, VOID = range(3)


class GoldenBatch:
    """1024 calls.  The procedures are the 61 entries of workloads.RPC_PROCS
    with flags 0; call i goes to procedure p = 7 i mod 61, whose argument type
    is p mod 3: record i of rec128_1024.xdr, record i of recvar_1024.xdr, or
    none.  One source per procedure, its entries in a fixed shuffled order,
    res = p.  300 calls are pending before: two runs and scattered values
    among the next 1024 after last_xid -- which wrap past 2^32 - 1 and meet a
    pending 0 -- and the rest far away."""

    N = 1024
    LAST_XID = 0xFFFFFE3F  # 448 values to the wrap

    def __init__(self):
        self.n = self.N
        self.procs = [tuple(int(v) for v in r[:3]) for r in W.RPC_PROCS if r[3] == 0]
        assert len(self.procs) == 61
        self.rec128 = g("rec128_1024.xdr")
        self.recvar = g("recvar_1024.xdr")
        self.varoffs = g("recvar_1024.offsets", "<u8")
        assert self.rec128.size == 128 * self.n and self.varoffs.size == self.n + 1
        self.proc = (7 * np.arange(self.n)) % 61
        self.kind = self.proc % 3
        rng = np.random.default_rng(12)
        near = np.concatenate([_run(self.LAST_XID + 5, 70), _run(0xFFFFFFF0, 40),  # the second run crosses the wrap
                               ((self.LAST_XID + 200 + 3 * np.arange(40)) & M32).astype(np.uint32)])
        far = rng.integers(0x1000, 0xF0000000, size=400, dtype=np.int64).astype(np.uint32)
        far = np.setdiff1d(far, near)[:300 - near.size]
        self.pending_xids = rng.permutation(np.concatenate([near, far]).astype(np.uint32))
        assert self.pending_xids.size == 300 == np.unique(self.pending_xids).size and 0 in self.pending_xids
        self.pending_res = rng.integers(61, size=300, dtype=np.int64).astype(np.uint32)
        self.xids = next_xids(self.pending_xids, self.LAST_XID, self.n)

    def record(self, kind: int, i: int) -> np.ndarray:
        if kind == REC128:
            return self.rec128[128 * i:128 * (i + 1)]
        if kind == RECVAR:
            return self.recvar[int(self.varoffs[i]):int(self.varoffs[i + 1])]
        return np.zeros(0, np.uint8)

    def source(self, p: int, n: int | None = None) -> Src:
        """Procedure p's source (n: only the calls below n, for a prefix)."""
        n = self.n if n is None else n
        calls = np.nonzero(self.proc[:n] == p)[0]
        calls = np.random.default_rng(1000 + p).permutation(calls).astype(np.uint64)
        kind = p % 3
        if kind == VOID:
            return Src(self.procs[p], p, calls)
        recs = [self.record(kind, int(i)) for i in calls]
        xdr = np.concatenate(recs + [np.zeros(0, np.uint8)])
        if kind == REC128:
            return Src(self.procs[p], p, calls, xdr, None, 128)
        return Src(self.procs[p], p, calls, xdr, np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.uint64))

    def sources(self, n: int | None = None) -> list:
        return [self.source(p, n) for p in range(61)]

    def expected(self, n: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """The stream assembled call by call, without model()."""
        n = self.n if n is None else n
        out = []
        for i in range(n):
            r = self.record(int(self.kind[i]), i)
            out.append(np.concatenate([call_header(int(self.xids[i]), self.procs[int(self.proc[i])], r.size), r]))
        offs = np.concatenate([[0], np.cumsum([m.size for m in out])]).astype(np.uint64)
        return np.concatenate(out), offs
