"""Host model of xdrg_rpc_recv_batch (test helper): msg_sock::input
(xdrpp/msgsock.cc:38-119) per connection, with the order of checks of
read_message (xdrpp/srpc.cc:29-55) that xdrg_index_msgs' ix_mark follows, and
rpc_sock::recv_msg's test (msgsock.cc:202-225).  Returns exactly what the call
returns: stream, offsets, conn_of, kind and the xdrg_rpc_conn records.
"""
from __future__ import annotations

import numpy as np

from xdrpp_amd import _abi as A

OPEN, FRAGMENT, TOO_LONG, BAD_SIZE, BAD_RPC = range(5)
LANE_BYTES = 1024   # kRbLaneBytes (recv_batch_kernels.h): a longer connection goes to the wave pass
WIN_BYTES = 16384   # kRbWinBytes: the wave pass's LDS window
TILE, SCAN_LANES = 256, 1024  # kTileThreads, kScanThreads (batch_kernels.h)
MAXLEN = A.MSG_SOCK_MAXMSGLEN


def frame(seg: np.ndarray, maxlen: int = MAXLEN, rpc: bool = False):
    """One connection: ([(pos, bytes, kind)], consumed, need, state)."""
    seg = np.asarray(seg, dtype=np.uint8)
    msgs, pos, n = [], 0, int(seg.size)
    while True:
        rem = n - pos
        if rem == 0:
            return msgs, pos, 0, OPEN                 # at a mark boundary: rdpos_ == 0, no rdmsg_
        if rem < 4:
            return msgs, pos, 4, OPEN                 # inside the mark: rdpos_ < 4 (msgsock.cc:68-81)
        if seg[pos] & 3:
            return msgs, pos, 0, BAD_SIZE             # the pre-swap size test (srpc.cc:38-39)
        v = int.from_bytes(seg[pos:pos + 4].tobytes(), "big")
        if not v & 0x80000000:
            return msgs, pos, 0, FRAGMENT             # msgsock.cc:86-91
        size = v & 0x7FFFFFFF
        if size > maxlen:
            return msgs, pos, 0, TOO_LONG             # msgsock.cc:99-117, from the mark alone
        if rem - 4 < size:
            return msgs, pos, 4 + size, OPEN          # inside the body: rdmsg_, rdpos_ (msgsock.cc:43-66)
        if size & 3:
            return msgs, pos, 0, BAD_SIZE             # xdr_get would throw (marshal.h:152-162)
        kind = 0
        if rpc:                                       # recv_msg (msgsock.cc:205-224)
            w1 = int.from_bytes(seg[pos + 8:pos + 12].tobytes(), "big") if size >= 8 else -1
            if w1 not in (0, 1):
                return msgs, pos, 0, BAD_RPC
            kind = w1
        msgs.append((pos, 4 + size, kind))
        pos += 4 + size


def recv_batch(buf: np.ndarray, segs, maxlen: int = MAXLEN, rpc: bool = False):
    """(stream, offsets[n + 1], conn_of, kind, conns) of the whole batch."""
    buf = np.asarray(buf, dtype=np.uint8)
    segs = np.asarray(segs).view(A.CONN_IN_DTYPE).reshape(-1)
    conns = np.zeros(len(segs), dtype=A.CONN_DTYPE)
    parts, offsets, conn_of, kind, at = [], [], [], [], 0
    for c, (b, ln) in enumerate(zip(segs["begin"].tolist(), segs["len"].tolist())):
        msgs, consumed, need, state = frame(buf[b:b + ln], maxlen, rpc)
        conns[c] = (len(offsets), consumed, len(msgs), need, state)
        offsets += [at + p for p, _, _ in msgs]
        conn_of += [c] * len(msgs)
        kind += [k for _, _, k in msgs]
        parts.append(buf[b:b + consumed])
        at += consumed
    stream = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return (stream, np.array(offsets + [at], dtype=np.uint64), np.array(conn_of, dtype=np.uint32),
            np.array(kind, dtype=np.uint8), conns)


# ------------------------------------------------------------ test inputs
def message(rng, size: int, frag: bool = False, word1: int | None = None) -> np.ndarray:
    m = rng.integers(0, 256, 4 + size, dtype=np.uint8)
    m[:4] = np.frombuffer((size | (0 if frag else 0x80000000)).to_bytes(4, "big"), dtype=np.uint8)
    if word1 is not None and size >= 8:
        m[8:12] = np.frombuffer(int(word1).to_bytes(4, "big"), dtype=np.uint8)
    return m


def connection(seed: int, sizes, frag=None, cut: int = 0, rpc_words: bool = True) -> np.ndarray:
    """A connection's bytes: messages of `sizes` body bytes with random
    bodies (word 1 CALL or REPLY when rpc_words), message `frag` without the
    last-fragment bit, `cut` bytes dropped from the end."""
    rng = np.random.default_rng(seed)
    ms = [message(rng, s, k == frag, int(rng.integers(0, 2)) if rpc_words else None) for k, s in enumerate(sizes)]
    x = np.concatenate(ms) if ms else np.zeros(0, np.uint8)
    return x[:x.size - cut] if cut else x


def pack(conn_bytes, align: int = 16):
    """Connections' bytes at `align`-aligned begins: (buf, segs)."""
    segs = np.zeros(len(conn_bytes), dtype=A.CONN_IN_DTYPE)
    at = 0
    for i, x in enumerate(conn_bytes):
        segs[i] = (at, x.size)
        at = (at + x.size + align - 1) // align * align
    buf = np.zeros(at, dtype=np.uint8)
    for s, x in zip(segs, conn_bytes):
        buf[int(s["begin"]):int(s["begin"]) + x.size] = x
    return buf, segs
