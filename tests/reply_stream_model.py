"""numpy model of xdrg_rpc_reply_batch (include/xdrgpu.h "Server reply
batch"): the reply stream srpc_server::run writes for a dispatched batch
(xdrpp/srpc.cc:83-88), restated from the contract.

Error replies come from the C restatement (oracle_bridge.rpc_replies, which
tests/test_rpc.py pins to the reference's fixtures); a success reply is the
reference's own header pattern (tests/golden/success_rec128_512.hdr7: the
mark and rpc_success_hdr of a void result) with the size and the xid put in,
then the result bytes.  GoldenBatch is the batch both test files use: the
reference's 1024 dispatched headers answered with the reference's encoded
rec128 / recvar records.
"""
import os
from typing import NamedTuple

import numpy as np

from conftest import GOLD

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
import oracle_bridge as O

MAX_MSG = A.MAX_MSG


def g(name, dtype=np.uint8):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


class Src(NamedTuple):
    """One xdrg_rpc_result_src on the host.  count: what *d_count holds (None:
    no d_count); len(index) is count_cap."""
    index: np.ndarray                 # uint64 message numbers
    xdr: np.ndarray | None = None     # None: void results
    offsets: np.ndarray | None = None  # None: fixed_size
    fixed_size: int = 0
    count: int | None = None

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
    def bytes_len(self) -> int:
        return 0 if self.xdr is None else int(self.xdr.size)


def success_header(xid: int, L: int) -> np.ndarray:
    w = g("success_rec128_512.hdr7").view(">u4").copy()
    assert w.tolist() == [24 | A.MARK_LAST, 7, 1, 0, 0, 0, 0]
    w[0] = (24 + L) | A.MARK_LAST
    w[1] = xid
    return w.view(np.uint8)


def usable(hdrs: np.ndarray, s: Src, k: int) -> bool:
    i = int(s.index[k])
    if i >= len(hdrs) or hdrs[i]["action"] != A.RPC_DISPATCH:
        return False
    a, b = s.span(k)
    if b < a or b > s.bytes_len or a % 4 or (b - a) % 4:
        return False
    return 24 + (b - a) <= MAX_MSG


def owners(hdrs: np.ndarray, sources: list) -> tuple[dict, int]:
    """{message: (source, position)} of the winning entries, and *d_unused."""
    own, entries = {}, 0
    for si, s in enumerate(sources):  # ascending (source, position): the first claim is the lowest
        for k in range(s.entries):
            entries += 1
            if usable(hdrs, s, k):
                own.setdefault(int(s.index[k]), (si, k))
    return own, entries - len(own)


def model(hdrs: np.ndarray, sources: list, capacity: int | None = None):
    """(stream, offsets uint64 [n + 1], unused, err): err is None or
    (XDRG_ERR_OVERFLOW_PUT, message); with an error the stream holds the
    replies before that message."""
    hdrs = np.ascontiguousarray(hdrs).view(R.HDR_DTYPE).reshape(-1)
    n = len(hdrs)
    own, unused = owners(hdrs, sources)
    estream, eoffs, rc, _ = O.rpc_replies(hdrs) if n else (np.zeros(0, np.uint8), np.zeros(1, np.uint64), 0, 0)
    assert rc == 0
    replies = []
    for i in range(n):
        if hdrs[i]["action"] == A.RPC_DISPATCH:
            if i in own:
                si, k = own[i]
                a, b = sources[si].span(k)
                body = sources[si].xdr[a:b] if b > a else np.zeros(0, np.uint8)
                replies.append(np.concatenate([success_header(int(hdrs[i]["xid"]), b - a), body]))
            else:
                replies.append(np.zeros(0, np.uint8))
        else:
            replies.append(estream[int(eoffs[i]):int(eoffs[i + 1])])
    offsets = np.concatenate([[0], np.cumsum([r.size for r in replies])]).astype(np.uint64)
    err, upto = None, n
    if capacity is not None:
        bad = [i for i in range(n) if replies[i].size and int(offsets[i + 1]) > capacity]
        if bad:
            err, upto = (A.ERR_OVERFLOW_PUT, bad[0]), bad[0]
    stream = np.concatenate(replies[:upto] + [np.zeros(0, np.uint8)])
    return stream, offsets, unused, err


# --------------------------------------------------------- the golden batch
REC128, RECVAR, VOID, UNSERVED = range(4)


class GoldenBatch:
    """rpccall_1024.hdrs (790 DISPATCH headers of 61 procedures, the error and
    dropped messages between them).  The procedures sorted, rank mod 4 picks
    the result type: rec128, recvar, void, unserved.  Message i of a served
    procedure answers with record i of rec128_1024.xdr / recvar_1024.xdr."""

    def __init__(self):
        self.hdrs = g("rpccall_1024.hdrs").view(R.HDR_DTYPE).copy()
        self.n = len(self.hdrs)
        self.rec128 = g("rec128_1024.xdr")
        self.recvar = g("recvar_1024.xdr")
        self.varoffs = g("recvar_1024.offsets", "<u8")
        assert self.rec128.size == 128 * self.n and self.varoffs.size == self.n + 1
        d = np.nonzero(self.hdrs["action"] == A.RPC_DISPATCH)[0]
        keys = [tuple(int(v) for v in self.hdrs["w"][i, 1:4]) for i in d]
        self.procs = sorted(set(keys))
        rank = {k: r for r, k in enumerate(self.procs)}
        self.kind = np.full(self.n, -1)
        self.proc = np.full(self.n, -1)
        for i, k in zip(d, keys):
            self.kind[i] = rank[k] % 4
            self.proc[i] = rank[k]

    def record(self, kind: int, i: int) -> np.ndarray:
        if kind == REC128:
            return self.rec128[128 * i:128 * (i + 1)]
        return self.recvar[int(self.varoffs[i]):int(self.varoffs[i + 1])]

    def source(self, kind: int, msgs, n: int | None = None) -> Src:
        """The results of kind `kind` for the messages `msgs`, in that order
        (n: only the messages below n, for a prefix of the batch)."""
        msgs = np.array([i for i in msgs if n is None or i < n], dtype=np.uint64)
        if kind == VOID:
            return Src(msgs)
        recs = [self.record(kind, int(i)) for i in msgs]
        xdr = np.concatenate(recs + [np.zeros(0, np.uint8)])
        if kind == REC128:
            return Src(msgs, xdr, None, 128)
        return Src(msgs, xdr, np.concatenate([[0], np.cumsum([r.size for r in recs])]).astype(np.uint64))

    def per_procedure(self, n: int | None = None) -> list:
        """One source per served procedure, entries in message order."""
        out = []
        for r in range(len(self.procs)):
            if r % 4 != UNSERVED:
                out.append(self.source(r % 4, np.nonzero(self.proc == r)[0], n))
        return out

    def per_type(self, n: int | None = None, seed: int = 3) -> list:
        """Three sources, one per result type, entries shuffled."""
        rng = np.random.default_rng(seed)
        return [self.source(k, rng.permutation(np.nonzero(self.kind == k)[0]), n) for k in (REC128, RECVAR, VOID)]

    def expected(self, n: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """The stream assembled from the reference's bytes alone, without the
        model: rpccall_1024.replies for the errors, the hdr7 pattern and the
        reference's encoded records for the successes."""
        n = self.n if n is None else n
        rep, ro = g("rpccall_1024.replies"), g("rpccall_1024.replyoffs", "<u8")
        out = []
        for i in range(n):
            k = self.kind[i]
            if k in (REC128, RECVAR):
                r = self.record(k, i)
                out.append(np.concatenate([success_header(int(self.hdrs[i]["xid"]), r.size), r]))
            elif k == VOID:
                out.append(success_header(int(self.hdrs[i]["xid"]), 0))
            else:
                out.append(rep[int(ro[i]):int(ro[i + 1])])
        offs = np.concatenate([[0], np.cumsum([m.size for m in out])]).astype(np.uint64)
        return np.concatenate(out), offs
