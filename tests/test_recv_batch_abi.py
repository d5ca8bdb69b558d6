"""CPU: the host side of the receive batch (include/xdrgpu.h "The receive
side"): the layouts of xdrg_rpc_conn_in and xdrg_rpc_conn and the
XDRG_CONN_* values read from the header, the workspace size, the argument
validation of xdrg_rpc_recv_batch that runs before any HIP call, the host
check of a segment table, and the Receiver helper against the model.  No GPU
call."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
import recv_model as RM

EINVAL, EALIGN, EUNSUPPORTED, ESPACE = -1, -2, -3, -6
FAKE = 0x10000  # a nonzero, 64 KiB-aligned address no call may dereference
FAR = 1 << 24

HEADER_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "xdrgpu.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("xdrg_rpc_conn_in %zu\n", sizeof(xdrg_rpc_conn_in));
  F(xdrg_rpc_conn_in, begin); F(xdrg_rpc_conn_in, len);
  printf("xdrg_rpc_conn %zu\n", sizeof(xdrg_rpc_conn));
  F(xdrg_rpc_conn, first); F(xdrg_rpc_conn, consumed); F(xdrg_rpc_conn, msgs); F(xdrg_rpc_conn, need);
  F(xdrg_rpc_conn, state);
  printf("OPEN %d\n", XDRG_CONN_OPEN);
  printf("FRAGMENT %d\n", XDRG_CONN_FRAGMENT);
  printf("TOO_LONG %d\n", XDRG_CONN_TOO_LONG);
  printf("BAD_SIZE %d\n", XDRG_CONN_BAD_SIZE);
  printf("BAD_RPC %d\n", XDRG_CONN_BAD_RPC);
  printf("RECV_RPC_SOCK %u\n", XDRG_RECV_RPC_SOCK);
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
    import ctypes as C
    for cname, ct, dt in (("xdrg_rpc_conn_in", A.XdrgRpcConnIn, A.CONN_IN_DTYPE),
                          ("xdrg_rpc_conn", A.XdrgRpcConn, A.CONN_DTYPE)):
        assert got[cname] == C.sizeof(ct) == dt.itemsize
        assert [f for f, _ in ct._fields_] == list(dt.names)
        for f, _ in ct._fields_:
            assert got[f"{cname}.{f}"] == getattr(ct, f).offset == dt.fields[f][1], (cname, f)
    assert (got["xdrg_rpc_conn_in"], got["xdrg_rpc_conn"]) == (16, 32)
    for k, v in {"OPEN": 0, "FRAGMENT": 1, "TOO_LONG": 2, "BAD_SIZE": 3, "BAD_RPC": 4}.items():
        assert got[k] == getattr(A, "CONN_" + k) == getattr(RM, k) == v
        assert R.CONN_STATE_NAMES[v] == k
    assert got["RECV_RPC_SOCK"] == A.RECV_RPC_SOCK == 1
    assert got["ABI"] == A.ABI_VERSION == A.lib().xdrg_abi_version() == 10


def test_workspace_size():
    need = A.lib().xdrg_rpc_recv_batch_workspace_size
    ns = (0, 1, 256, 257, 1 << 16, RM.TILE * RM.SCAN_LANES + 1, 1 << 31)
    sizes = [need(n, 1 << 20) for n in ns]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes), sizes
    # per connection a base and a list entry, per tile two sums
    assert all(s >= 12 * n + 16 * ((n + RM.TILE - 1) // RM.TILE) for s, n in zip(sizes, ns))
    assert sizes[1] > sizes[0] and sizes[3] > sizes[2]
    for n in ns:  # monotone in the buffer's length too
        by_len = [need(n, b) for b in (0, 1, 1 << 20, 1 << 40)]
        assert by_len == sorted(by_len)


def recv(buf=FAKE, buf_len=4096, segs=FAR, nconns=3, maxlen=1 << 20, flags=1, out=2 * FAR, cap=4096,
         offsets=3 * FAR, max_msgs=1024, count=4 * FAR, conn_of=5 * FAR, kind=6 * FAR, conns=7 * FAR, ws=8 * FAR,
         ws_bytes=1 << 40, status=9 * FAR):
    return A.lib().xdrg_rpc_recv_batch(buf, buf_len, segs, nconns, maxlen, flags, out, cap, offsets, max_msgs, count,
                                       conn_of, kind, conns, ws, ws_bytes, status, None)


def test_recv_batch_validates_before_any_hip_call():
    # every refusal below comes before the workspace test, which comes before the first launch
    assert recv(ws_bytes=0) == ESPACE
    for name in ("segs", "conns", "offsets", "count", "status", "buf", "out", "conn_of", "kind"):
        assert recv(**{name: None}) == EINVAL, name
    assert recv(kind=None, flags=0, ws_bytes=0) == ESPACE      # without the flag d_kind may be NULL
    assert recv(flags=2) == EINVAL and recv(flags=3) == EINVAL
    # d_out against d_buf: equal, overlapping from either side, and just clear of it
    assert recv(out=FAKE) == EINVAL
    assert recv(out=FAKE + 4092) == EINVAL
    assert recv(out=FAKE - 4092) == EINVAL
    assert recv(out=FAKE + 4096, ws_bytes=0) == ESPACE
    assert recv(out=FAKE - 4096, ws_bytes=0) == ESPACE
    # alignment: the byte streams and d_conn_of 4, every other array 8
    assert recv(buf=FAKE + 2) == EALIGN and recv(out=2 * FAR + 1) == EALIGN and recv(conn_of=5 * FAR + 2) == EALIGN
    assert recv(buf=FAKE + 4, out=2 * FAR + 4, conn_of=5 * FAR + 4, ws_bytes=0) == ESPACE
    for name, v in (("segs", FAR), ("offsets", 3 * FAR), ("count", 4 * FAR), ("conns", 7 * FAR), ("ws", 8 * FAR),
                    ("status", 9 * FAR)):
        assert recv(**{name: v + 4}) == EALIGN, name
    assert recv(kind=6 * FAR + 1, ws_bytes=0) == ESPACE         # bytes: any address
    # limits
    assert recv(nconns=1 << 31) == EUNSUPPORTED and recv(max_msgs=1 << 40) == EUNSUPPORTED
    need = A.lib().xdrg_rpc_recv_batch_workspace_size
    assert recv(ws_bytes=need(3, 4096) - 1) == ESPACE and recv(ws=None) == ESPACE
    assert recv(nconns=257, ws_bytes=need(257, 4096) - 1) == ESPACE


def test_segment_table_is_checked_where_the_host_sees_it():
    """xdrg_rpc_recv_batch's table lives on the device; recv_batch() takes a
    host table and refuses a violated one with EINVAL before anything is sent
    to the GPU (a CPU tensor here: a launch would fail differently)."""
    import torch
    buf = torch.zeros(256, dtype=torch.uint8)
    ok = np.array([(0, 13), (16, 0), (16, 7), (24, 232)], dtype=A.CONN_IN_DTYPE)
    assert np.array_equal(R.check_segs(ok, 256), ok)
    assert np.array_equal(R.check_segs([[0, 13], [16, 0]], 256), ok[:2])
    for bad in ([(2, 8)],                      # begin not a multiple of 4
                [(0, 16), (17, 4)],            # the second begin
                [(0, 20), (16, 4)],            # overlapping
                [(16, 4), (0, 8)],             # descending
                [(0, 8), (200, 57)],           # past the buffer
                [(260, 0)],
                [(0, (1 << 64) - 4)]):         # no wrap-around
        with pytest.raises(A.AbiError, match="EINVAL"):
            R.recv_batch(buf, np.array(bad, dtype=A.CONN_IN_DTYPE))


def test_receiver_against_the_model():
    """Receiver is the host's rdpos_ / rdmsg_: fed in pieces and advanced by
    the model's records, it delivers what one read of everything delivers."""
    rng = np.random.default_rng(9)
    conns = {"a": RM.connection(1, [8, 40, 0, 8]), "b": RM.connection(2, [100] * 3), "c": RM.connection(3, [8, 8]),
             "d": RM.connection(4, [8, 8, 8], frag=1), "e": np.zeros(0, np.uint8)}
    rx = R.Receiver()
    got = {k: [] for k in conns}
    at = {k: 0 for k in conns}
    held_back = 0
    for rnd in range(8):
        for k, x in conns.items():
            if k in rx.closed or at[k] >= x.size:
                continue
            n = x.size - at[k] if rnd == 7 else int(rng.integers(0, 60))
            rx.feed(k, x[at[k]:at[k] + n].tobytes())
            at[k] += n
        buf, segs = rx.batch(pin=False)
        ids = rx.ids
        assert (segs["begin"] % 16 == 0).all() and buf.dtype.itemsize == 1
        R.check_segs(segs, buf.numel())
        held_back += sum(1 for k in conns if rx.pending(k) and k not in ids)
        stream, offsets, conn_of, _, recs = RM.recv_batch(buf.numpy(), segs)
        for i, k in enumerate(ids):
            f, n = int(recs["first"][i]), int(recs["msgs"][i])
            got[k] += [stream[int(offsets[j]):int(offsets[j + 1])].tobytes() for j in range(f, f + n)]
        rx.advance(recs)
    assert held_back > 0
    for k, x in conns.items():
        msgs, consumed, _, state = RM.frame(x)
        assert got[k] == [x[p:p + b].tobytes() for p, b, _ in msgs], k
        assert (rx.closed.get(k, RM.OPEN) == state) and (state != RM.OPEN or rx.pending(k) == 0)
    assert rx.closed == {"d": RM.FRAGMENT}
    with pytest.raises(ValueError, match="closed"):
        rx.feed("d", b"\x00")


def test_reply_ranges_tile_a_reply_stream():
    import torch
    recs = np.array([(0, 24, 2, 0, 0), (2, 0, 0, 4, 0), (2, 12, 1, 0, 1), (3, 36, 3, 0, 0)], dtype=A.CONN_DTYPE)
    got = R.Received(torch.zeros(0, dtype=torch.uint8), torch.zeros(7, dtype=torch.int64), 6,
                     torch.zeros(6, dtype=torch.int32), None, torch.from_numpy(recs.view(np.int64).copy()))
    reply_offsets = torch.tensor([0, 28, 28, 60, 96, 96, 124], dtype=torch.int64)
    r = got.reply_ranges(reply_offsets)
    assert r.tolist() == [[0, 28], [28, 28], [28, 60], [60, 124]]
    assert (r[1:, 0] == r[:-1, 1]).all()
