"""CPU: the host side of the send batch (include/xdrgpu.h "The send side"):
the layouts of xdrg_rpc_send_src and xdrg_rpc_wqueue read from the header, the
workspace size, the argument validation of xdrg_rpc_send_batch that runs
before any HIP call, and the Sender helper against the model (msg_sock's
putmsg, pop_wbytes and output restated in tests/send_model.py).  No GPU call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
import send_model as SM

EINVAL, EALIGN, EUNSUPPORTED, ESPACE = -1, -2, -3, -6
FAKE = 0x10000  # a nonzero, 64 KiB-aligned address no call may dereference
FAR = 1 << 24

HEADER_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "xdrgpu.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("xdrg_rpc_send_src %zu\n", sizeof(xdrg_rpc_send_src));
  F(xdrg_rpc_send_src, d_bytes); F(xdrg_rpc_send_src, d_offsets); F(xdrg_rpc_send_src, d_conn);
  F(xdrg_rpc_send_src, d_count); F(xdrg_rpc_send_src, bytes_len); F(xdrg_rpc_send_src, count_cap);
  F(xdrg_rpc_send_src, conn);
  printf("xdrg_rpc_wqueue %zu\n", sizeof(xdrg_rpc_wqueue));
  F(xdrg_rpc_wqueue, first); F(xdrg_rpc_wqueue, msgs); F(xdrg_rpc_wqueue, begin); F(xdrg_rpc_wqueue, len);
  printf("MAX_SEND_SRCS %u\n", XDRG_RPC_MAX_SEND_SRCS);
  printf("SEND_SORT_TILE %u\n", XDRG_RPC_SEND_SORT_TILE);
  printf("ABI %d\n", XDRG_ABI_VERSION);
  return 0;
}
"""


def test_header_facts(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(HEADER_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert A.SEND_SRC is A.XdrgRpcSendSrc and R.WQUEUE_DTYPE is A.WQUEUE_DTYPE
    for f, _ in A.XdrgRpcSendSrc._fields_:
        assert got[f"xdrg_rpc_send_src.{f}"] == getattr(A.XdrgRpcSendSrc, f).offset, f
    assert [f for f, _ in A.XdrgRpcWqueue._fields_] == list(A.WQUEUE_DTYPE.names)
    for f, _ in A.XdrgRpcWqueue._fields_:
        assert got[f"xdrg_rpc_wqueue.{f}"] == getattr(A.XdrgRpcWqueue, f).offset == A.WQUEUE_DTYPE.fields[f][1], f
    assert got["xdrg_rpc_send_src"] == C.sizeof(A.XdrgRpcSendSrc) == 48
    assert got["xdrg_rpc_wqueue"] == C.sizeof(A.XdrgRpcWqueue) == A.WQUEUE_DTYPE.itemsize == 32
    assert got["MAX_SEND_SRCS"] == A.RPC_MAX_SEND_SRCS == 64
    assert got["SEND_SORT_TILE"] == A.RPC_SEND_SORT_TILE == SM.SORT_TILE
    assert got["ABI"] == A.ABI_VERSION == A.lib().xdrg_abi_version() == 10
    assert (A.SEND_DROPPED, A.SEND_EMPTY, A.SEND_UNUSABLE) == (SM.DROPPED, SM.EMPTY, SM.UNUSABLE) == (-1, -2, -3)
    for name in ("xdrg_rpc_send_batch", "xdrg_rpc_send_batch_workspace_size"):
        assert name in A.EXPORTED and hasattr(A.lib(), name)


def test_workspace_size():
    need = A.lib().xdrg_rpc_send_batch_workspace_size
    ns = (0, 1, 256, 257, SM.SORT_TILE, SM.SORT_TILE + 1, 1 << 20, 0xffffffff)
    for nconns in (0, 1, 255, 256, 65535, 65536, (1 << 24) + 1, 0x7fffffff):
        sizes = [need(n, nconns) for n in ns]
        assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes), sizes
        assert sizes[0] > 0                                   # zero entries still need the control words
        assert all(s >= 8 * n for s, n in zip(sizes, ns))     # an item per entry
    for n in ns:  # monotone in the connections too: more digits, never less room
        by_conns = [need(n, c) for c in (0, 1, 255, 256, 65535, 65536, 1 << 24, 0x7fffffff)]
        assert by_conns == sorted(by_conns)
    assert need(1 << 20, 2) >= 2 * 8 * (1 << 20)              # both sides of a pass


def srcs(*rows):
    """A HOST array of xdrg_rpc_send_src from (bytes, offsets, conn, count, bytes_len, cap, conn_all) rows."""
    arr = (A.XdrgRpcSendSrc * max(len(rows), 1))()
    for k, r in enumerate(rows):
        arr[k] = A.XdrgRpcSendSrc(*r)
    return arr


GOOD = (FAKE, FAR, 2 * FAR, 3 * FAR, 4096, 100, 0)


def send(rows=(GOOD,), nsrcs=None, nconns=3, closed=4 * FAR, out=5 * FAR, cap=4096, offsets=6 * FAR, count=7 * FAR,
         conn_of=8 * FAR, origin=9 * FAR, pos=10 * FAR, queues=11 * FAR, counts=12 * FAR, ws=13 * FAR,
         ws_bytes=1 << 40, status=14 * FAR, table=True):
    return A.lib().xdrg_rpc_send_batch(srcs(*rows) if table else None, len(rows) if nsrcs is None else nsrcs, nconns,
                                       closed, out, cap, offsets, count, conn_of, origin, pos, queues, counts, ws,
                                       ws_bytes, status, None)


def with_(i, v):
    r = list(GOOD)
    r[i] = v
    return (tuple(r),)


def test_send_batch_validates_before_any_hip_call():
    # every refusal below comes before the workspace test, which comes before the first launch
    assert send(ws_bytes=0) == ESPACE
    for name in ("offsets", "count", "status", "out", "conn_of", "origin", "queues"):
        assert send(**{name: None}) == EINVAL, name
    assert send(table=False) == EINVAL
    for name in ("closed", "pos", "counts"):                 # may be NULL
        assert send(**{name: None}, ws_bytes=0) == ESPACE, name
    assert send(out=None, cap=0, ws_bytes=0) == ESPACE and send(queues=None, nconns=0, ws_bytes=0) == ESPACE
    assert send(rows=(), conn_of=None, origin=None, table=False, ws_bytes=0) == ESPACE   # no entries: nothing to name
    assert send(rows=(GOOD,) * 64, ws_bytes=0) == ESPACE and send(rows=(GOOD,) * 65) == EINVAL
    assert send(nsrcs=65) == EINVAL
    # a source
    assert send(rows=with_(1, None)) == EINVAL               # entries without offsets
    assert send(rows=(GOOD[:1] + (None,) + GOOD[2:5] + (0, 0),), ws_bytes=0) == ESPACE   # none: no offsets needed
    assert send(rows=with_(0, None)) == EINVAL               # bytes_len without bytes
    assert send(rows=with_(2, None), ws_bytes=0) == ESPACE   # d_conn NULL: every entry goes to `conn`
    assert send(rows=with_(3, None), ws_bytes=0) == ESPACE   # d_count NULL: count_cap entries
    # d_out against a source's bytes: equal, overlapping from either side, and just clear of it
    for out, rc in ((FAKE, EINVAL), (FAKE + 4092, EINVAL), (FAKE - 4092, EINVAL), (FAKE + 4096, ESPACE),
                    (FAKE - 4096, ESPACE)):
        assert send(out=out, ws_bytes=0) == rc, hex(out)
    assert send(rows=(GOOD, (5 * FAR + 8,) + GOOD[1:])) == EINVAL   # the second source's
    # alignment: the byte streams and the u32 arrays 4, every other array 8
    for name, v in (("closed", 4 * FAR), ("out", 5 * FAR), ("conn_of", 8 * FAR)):
        assert send(**{name: v + 2}) == EALIGN, name
        assert send(**{name: v + 4}, ws_bytes=0) == ESPACE, name
    for name, v in (("offsets", 6 * FAR), ("count", 7 * FAR), ("origin", 9 * FAR), ("pos", 10 * FAR),
                    ("queues", 11 * FAR), ("counts", 12 * FAR), ("ws", 13 * FAR), ("status", 14 * FAR)):
        assert send(**{name: v + 4}) == EALIGN, name
    for i, off, rc in ((0, 2, EALIGN), (0, 4, ESPACE), (2, 2, EALIGN), (2, 4, ESPACE), (1, 4, EALIGN), (3, 4, EALIGN)):
        assert send(rows=with_(i, GOOD[i] + off), ws_bytes=0 if rc == ESPACE else 1 << 40) == rc, (i, off)
    # limits
    big = with_(5, 0xffffffff)
    assert send(rows=big, ws_bytes=0) == ESPACE and send(rows=big + (GOOD[:5] + (1, 0),)) == EUNSUPPORTED
    assert send(nconns=0x7fffffff, ws_bytes=0) == ESPACE and send(nconns=1 << 31) == EUNSUPPORTED
    need = A.lib().xdrg_rpc_send_batch_workspace_size
    assert send(ws_bytes=need(100, 3) - 1) == ESPACE and send(ws=None) == ESPACE
    assert send(nconns=300, ws_bytes=need(100, 300) - 1) == ESPACE
    assert send(rows=(GOOD, GOOD), ws_bytes=need(200, 3) - 1) == ESPACE   # the sum of count_cap


def test_python_layer_refuses_what_the_host_sees():
    e = torch.zeros(0, dtype=torch.uint8)
    o = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="at most 64"):
        R.send_batch([R.send_source(e, o, 0)] * 65, 1)
    s = R.send_source(torch.zeros(8, dtype=torch.uint8), torch.tensor([0, 4, 8]), [1, 0])
    assert s.cap == 2 and s.conn.dtype == torch.int32 and R.send_source(e, o, 3).conn == 3
    with pytest.raises(ValueError, match="one socket number per call"):
        R.send_source(torch.zeros(8, dtype=torch.uint8), torch.tensor([0, 4, 8]), [1, 0, 2])


# ------------------------------------------------------------------ Sender
def queued_of(model: dict) -> R.Queued:
    """The model's result as send_batch() would return it (host tensors)."""
    return R.Queued(torch.from_numpy(model["stream"].copy()), torch.from_numpy(model["offsets"].view(np.int64).copy()),
                    model["count"], torch.from_numpy(model["conn_of"].view(np.int32).copy()),
                    torch.from_numpy(model["origin"].view(np.int64).copy()), torch.from_numpy(model["pos"].copy()),
                    torch.from_numpy(model["queues"].view(np.int64).copy()), model["counts"])


def same_sock(tx: R.Sender, conn, ms: SM.MsgSock, maxiov=8):
    assert tx.pending(conn) == ms.wsize
    assert [bytes(v) for v in tx.iov(conn, maxiov)] == ms.iov(maxiov)
    assert (conn in tx.failed) == ms.wfail


def test_sender_against_the_model():
    """Sender is the host's wqueue_ / wstart_ / wsize_ / wfail_: three rounds
    of send_batch's queues (the model's), and between them seeded writes that
    end inside a mark, inside a body, exactly at a boundary and across many
    messages, EAGAIN, a failure with a queue outstanding and putmsg after it."""
    rng = np.random.default_rng(11)
    nconns = 9
    ids = [f"c{c}" for c in range(nconns)]
    tx = R.Sender()
    socks = {i: SM.MsgSock() for i in ids}
    seen = {"mark": 0, "body": 0, "boundary": 0, "many": 0, "eagain": 0, "fail_queued": 0, "dropped": 0, "all": 0}
    for rnd in range(3):
        msgs = [SM.message(rng, 4 * int(rng.integers(0, 12)), tag=rnd * 1000 + i) for i in range(120)]
        conn = rng.integers(0, nconns, 120)
        closed = tx.closed(nconns, ids)
        assert closed.dtype == torch.int32 and closed.tolist() == [int(socks[i].wfail) for i in ids]
        model = SM.send_batch([SM.source(msgs[:70], conn[:70]), SM.source(msgs[70:], conn[70:])], nconns)
        tx.queue(queued_of(model), ids)
        for i, c in zip(range(120), conn):                   # putmsg in ascending global number
            seen["dropped"] += socks[ids[c]].wfail
            socks[ids[c]].putmsg(msgs[i].tobytes())
        for i in ids:
            same_sock(tx, i, socks[i])
            same_sock(tx, i, socks[i], maxiov=3)
        for step in range(40):
            i = ids[int(rng.integers(0, nconns))]
            ms = socks[i]
            v = ms.iov()
            offered = sum(len(b) for b in v)
            if not offered:
                continue
            kind = int(rng.integers(0, 10))
            if kind == 0:                                     # EAGAIN: nothing changes
                ms.output(-1, eagain=True)
                seen["eagain"] += 1
            else:
                front = len(v[0])
                n = {2: min(2, offered), 3: min(front, 6) if front > 4 else front, 4: front, 5: offered}.get(
                    kind, int(rng.integers(1, offered + 1)))
                seen["mark"] += n < front and ms.wstart + n < 4
                seen["body"] += n < front and ms.wstart + n > 4
                seen["boundary"] += n == front
                seen["many"] += len(v) > 2 and n > front + len(v[1])
                seen["all"] += n == ms.wsize
                ms.output(n)
                tx.wrote(i, n)
            same_sock(tx, i, ms)
        if rnd < 2:                                           # ECONNRESET with a queue outstanding
            i = next(i for i in ids if socks[i].wsize and len(socks[i].wqueue) > 1)
            seen["fail_queued"] += 1
            socks[i].output(-1, eagain=False)
            tx.fail(i)
            same_sock(tx, i, socks[i])
    assert all(v > 0 for v in seen.values()), seen
    with pytest.raises(ValueError, match="queued"):
        live = next(i for i in ids if socks[i].wsize)
        tx.wrote(live, socks[live].wsize + 1)
    tx.wrote(live, 0)
    dead = next(i for i in ids if socks[i].wfail)
    tx.putmsg(dead, b"\x80\x00\x00\x00")
    assert tx.pending(dead) == 0 and tx.iov(dead) == []


def test_model_on_a_literal_batch():
    """The model against a batch small enough to work out by hand: two
    sources, three connections, one closed, every outcome once."""
    m = lambda body, tag: SM.message(np.random.default_rng(tag), body, tag)
    a = SM.source([m(4, 1), np.zeros(0, np.uint8), m(8, 2), m(0, 3)], [2, 0, 0, 1])
    b = SM.source([m(4, 4), m(4, 5), m(12, 6)], [0, 7, 2])
    b["bytes"][b["offsets"][2].astype(int) + 3] ^= 1          # the third's mark no longer matches its length
    r = SM.send_batch([a, b], 3, closed=[0, 1, 0])
    # g:      0 (conn 2)  1 empty  2 (conn 0)  3 dropped  4 (conn 0)  5 conn 7  6 bad mark
    assert r["pos"].tolist() == [2, SM.EMPTY, 0, SM.DROPPED, 1, SM.UNUSABLE, SM.UNUSABLE]
    assert r["counts"] == (3, 1, 1, 2) and r["count"] == 3
    assert r["conn_of"].tolist() == [0, 0, 2] and r["origin"].tolist() == [2, (1 << 32) | 0, 0]
    assert r["offsets"].tolist() == [0, 12, 20, 28]
    assert r["stream"].tobytes() == a["bytes"][8:20].tobytes() + b["bytes"][:8].tobytes() + a["bytes"][:8].tobytes()
    assert r["queues"].tolist() == [(0, 2, 0, 20), (2, 0, 20, 0), (2, 1, 20, 8)]
    short = SM.send_batch([a, b], 3, closed=[0, 1, 0], capacity=19)
    assert (short["code"], short["record"]) == (A.ERR_OVERFLOW_PUT, 1) and short["stream"].size == 12
    assert short["queues"].tolist() == r["queues"].tolist() and short["total_bytes"] == 28
