"""Host model of xdrg_rpc_send_batch and of Sender (test helper):
msg_sock::putmsg, pop_wbytes and output (xdrpp/msgsock.cc:121-188) restated
per connection, and the batch as the contract of include/xdrgpu.h "The send
side" states it: the outcome of every entry, then a stable argsort of the keys.
Returns exactly what the call returns.
"""
from __future__ import annotations

from collections import deque

import numpy as np

from xdrpp_amd import _abi as A

DROPPED, EMPTY, UNUSABLE = -1, -2, -3
SORT_TILE = A.RPC_SEND_SORT_TILE  # kSbSortTile (send_batch_kernels.h)
TILE, SCAN_LANES = 256, 1024       # kTileThreads, kScanThreads (batch_kernels.h)


# ------------------------------------------------------------ one connection
class MsgSock:
    """wqueue_, wstart_, wsize_ and wfail_ of one msg_sock, line by line."""

    def __init__(self):
        self.wqueue, self.wstart, self.wsize, self.wfail = deque(), 0, 0, False

    def putmsg(self, mb: bytes) -> None:          # msgsock.cc:121-134, without the output() it starts
        if self.wfail:                            # :124-127
            return
        self.wsize += len(mb)                     # :130
        self.wqueue.append(bytes(mb))             # :131

    def pop_wbytes(self, n: int) -> None:         # :136-155
        if n == 0:
            return
        assert n <= self.wsize
        self.wsize -= n
        frontbytes = len(self.wqueue[0]) - self.wstart
        if n < frontbytes:
            self.wstart += n
            return
        n -= frontbytes
        self.wqueue.popleft()
        while n > 0 and n >= len(self.wqueue[0]):
            n -= len(self.wqueue[0])
            self.wqueue.popleft()
        self.wstart = n

    def iov(self, maxiov: int = 8) -> list:       # :160-172
        v = []
        for i, b in enumerate(self.wqueue):
            if i >= maxiov:
                break
            v.append(b if i else b[self.wstart:])
        return v

    def output(self, n, eagain: bool = False) -> None:
        """What output() does with writev's return value n (:173-182)."""
        if n <= 0:
            if n != -1 or not eagain:
                self.wfail = True
                self.wsize = self.wstart = 0
                self.wqueue.clear()
            return
        self.pop_wbytes(n)


# ------------------------------------------------------------------ sources
def message(rng, body: int, tag: int | None = None) -> np.ndarray:
    """One record-marked message of `body` bytes (a multiple of 4) after the
    mark; with a tag its first body word is the tag, the rest is random."""
    m = np.empty(4 + body, dtype=np.uint8)
    m[:4] = np.frombuffer((body | A.MARK_LAST).to_bytes(4, "big"), dtype=np.uint8)
    m[4:] = rng.integers(0, 256, body, dtype=np.uint8)
    if tag is not None and body >= 4:
        m[4:8] = np.frombuffer(int(tag).to_bytes(4, "big"), dtype=np.uint8)
    return m


def source(msgs, conn, count=None, cap=None) -> dict:
    """A source from a list of byte arrays (an empty one is an empty entry):
    bytes, offsets uint64 [len + 1], conn (uint32 array or int), count (the
    device count, or None), cap."""
    sizes = np.array([len(m) for m in msgs], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    data = np.concatenate([np.asarray(m, dtype=np.uint8) for m in msgs]) if len(msgs) else np.zeros(0, np.uint8)
    if not isinstance(conn, (int, np.integer)):
        conn = np.asarray(conn).astype(np.uint32)
    return {"bytes": data, "offsets": offsets, "conn": conn, "count": count, "cap": len(msgs) if cap is None else cap}


def marks_source(n: int, conn) -> dict:
    """n bare marks (4-byte messages), built with array operations."""
    data = np.zeros((n, 4), dtype=np.uint8)
    data[:, 0] = 0x80
    return {"bytes": data.reshape(-1), "offsets": np.arange(n + 1, dtype=np.uint64) * 4,
            "conn": np.asarray(conn).astype(np.uint32), "count": None, "cap": n}


def outcomes(src: dict, nconns: int, closed):
    """Per entry of one source (cap of them): pos code (0 for queued), conn,
    begin, length, used."""
    cap = src["cap"]
    data, offs = src["bytes"], np.asarray(src["offsets"], dtype=np.uint64)
    used = np.arange(cap) < (cap if src["count"] is None else min(int(src["count"]), cap))
    a, b = offs[:cap], offs[1:cap + 1]
    conn = np.full(cap, src["conn"], dtype=np.uint32) if isinstance(src["conn"], (int, np.integer)) \
        else np.asarray(src["conn"], dtype=np.uint32)[:cap]
    code = np.zeros(cap, dtype=np.int64)
    length = np.where(b >= a, b - a, np.uint64(0))
    bad = (b < a) | (b > np.uint64(data.size)) | (((a | b) & np.uint64(3)) != 0) | (length < 4) | \
        (length > np.uint64(4 + A.MAX_MSG)) | (conn >= nconns)
    # the first word, where the span can be read at all
    can = ~bad & (a != b)
    words = np.zeros(cap, dtype=np.uint64)
    if can.any():
        idx = a[can].astype(np.int64)
        quad = data[idx[:, None] + np.arange(4)].astype(np.uint64)
        words[can] = (quad[:, 0] << 24) | (quad[:, 1] << 16) | (quad[:, 2] << 8) | quad[:, 3]
    bad |= can & (words != ((length - np.uint64(4)) | np.uint64(A.MARK_LAST)))
    if closed is not None:
        shut = np.asarray(closed)[np.minimum(conn, max(nconns - 1, 0))] != 0 if nconns else np.zeros(cap, bool)
        code[shut] = DROPPED
    code[bad] = UNUSABLE
    code[a == b] = EMPTY
    code[~used] = EMPTY
    return code, conn, a, length, used


def send_batch(sources, nconns: int, closed=None, capacity: int | None = None) -> dict:
    """The whole call: stream, offsets [m + 1], conn_of, origin, pos, queues,
    counts, total_bytes, and (code, record) for a capacity below the total (the
    stream then holds the messages before `record` only)."""
    codes, conns, begins, lengths, useds, srcno, entno, bases = [], [], [], [], [], [], [], []
    base = 0
    for s, src in enumerate(sources):
        code, conn, a, ln, used = outcomes(src, nconns, closed)
        codes.append(code); conns.append(conn); begins.append(a); lengths.append(ln); useds.append(used)
        srcno.append(np.full(src["cap"], s, dtype=np.uint64))
        entno.append(np.arange(src["cap"], dtype=np.uint64))
        bases.append(base)
        base += src["bytes"].size
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    code, conn, begin, length, used = cat(codes, np.int64), cat(conns, np.uint32), cat(begins, np.uint64), \
        cat(lengths, np.uint64), cat(useds, bool)
    src_of, ent_of = cat(srcno, np.uint64), cat(entno, np.uint64)
    queued = code == 0
    keys = np.where(queued, conn.astype(np.int64), nconns)
    order = np.argsort(keys, kind="stable")           # putmsg order: ascending global number on every connection
    m = int(queued.sum())
    g = order[:m]
    pos = code.copy()
    pos[g] = np.arange(m)
    sizes = length[g]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(offsets[-1])
    # the gather: byte i of the stream comes from the concatenated sources
    allbytes = np.concatenate([s["bytes"] for s in sources]) if sources else np.zeros(0, np.uint8)
    fit = m
    if capacity is not None and capacity < total:
        fit = int(np.searchsorted(offsets[1:], capacity, side="right"))  # the first position whose end is past it
    starts = np.array(bases, dtype=np.int64)[src_of[g[:fit]].astype(np.int64)] + begin[g[:fit]].astype(np.int64) \
        if fit else np.zeros(0, np.int64)
    lens = sizes[:fit].astype(np.int64)
    nbytes = int(lens.sum())
    idx = np.repeat(starts - offsets[:fit].astype(np.int64), lens) + np.arange(nbytes)
    stream = allbytes[idx] if nbytes else np.zeros(0, np.uint8)
    queues = np.zeros(nconns, dtype=A.WQUEUE_DTYPE)
    skeys = keys[g]
    lo = np.searchsorted(skeys, np.arange(nconns), side="left")
    hi = np.searchsorted(skeys, np.arange(nconns), side="right")
    queues["first"], queues["msgs"] = lo, hi - lo
    queues["begin"], queues["len"] = offsets[lo], offsets[hi] - offsets[lo]
    counts = (m, int(((code == DROPPED) & used).sum()), int(((code == EMPTY) & used).sum()),
              int(((code == UNUSABLE) & used).sum()))
    return {"stream": stream, "offsets": offsets, "count": m, "conn_of": conn[g].astype(np.uint32),
            "origin": (src_of[g] << np.uint64(32)) | ent_of[g], "pos": pos, "queues": queues, "counts": counts,
            "total_bytes": total, "code": A.ERR_OVERFLOW_PUT if fit < m else 0, "record": fit if fit < m else None,
            "keys": keys}
