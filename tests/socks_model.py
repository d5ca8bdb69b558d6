"""TEST INFRASTRUCTURE for tests/test_socks_abi.py and test_gpu_socks.py: a
model of the many-socket client calls (include/xdrgpu.h "The asynchronous
client over many connections").

The literal restatement: every connection is its own rpc_sock, so the state is
a dict {socket: calls_} of dicts {xid: caller position} and a dict of xid_
values.  get_xid and send_call (xdrpp/msgsock.h:118-122, msgsock.cc:227-232)
are call_stream_model.next_xids and .merge on one socket's dict at a time;
recv_msg (msgsock.cc:202-232) looks a reply up in the dict of the socket it
arrived on; the callback's call_result and the erases are settle_model's, one
socket at a time, and abort_all_calls (msgsock.cc:190-200) clears the dict of
the socket it runs on and of no other.

Arrays named `tsock` / `table` are in table order (sorted by (sock, xid));
everything else names a call by its position in the caller's arrays.
"""
from __future__ import annotations

import numpy as np

import call_stream_model as CS
import oracle_bridge as O
import reply_model as RM
import settle_model as SM
from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R

NO_CALL = SM.NO_CALL
M32 = CS.M32


def u32(v) -> np.ndarray:
    return (np.asarray(v).astype(np.int64).reshape(-1) & M32).astype(np.uint32)


def sorted_table(socks, xids, res):
    """(tsock int64, table CALL_DTYPE, perm: table position -> caller's)."""
    x, g = u32(xids), np.broadcast_to(np.asarray(socks).astype(np.int64), u32(xids).shape)
    r = np.broadcast_to(u32(res) if np.ndim(res) else np.uint32(res), x.shape)
    order = np.lexsort((x, g))
    t = np.zeros(x.size, dtype=R.CALL_DTYPE)
    t["xid"], t["res"] = x[order], r[order]
    return g[order].astype(np.int64), t, order.astype(np.int64)


def run_of(sorted_socks, g: int) -> tuple[int, int]:
    s = np.asarray(sorted_socks).astype(np.int64)
    return int(np.searchsorted(s, g, "left")), int(np.searchsorted(s, g, "right"))


def socks_of(*arrays) -> list[int]:
    return sorted(set(int(v) for a in arrays for v in np.asarray(a).reshape(-1)))


# ------------------------------------------------------ get_xid, send_call
def next_xids(tsock, table, last, call_sock):
    """(xids uint32 [n], last_out uint32 [nsocks]): every socket's get_xid
    loop over its own calls_.  A socket number that is no socket counts from
    0."""
    last = u32(last)
    cs = np.asarray(call_sock).astype(np.int64)
    assert (np.diff(cs) >= 0).all()
    xids = np.zeros(cs.size, dtype=np.uint32)
    last_out = last.copy()
    for g in socks_of(cs):
        a, b = run_of(cs, g)
        lo, hi = run_of(tsock, g)
        xids[a:b] = CS.next_xids(table["xid"][lo:hi], int(last[g]) if g < last.size else 0, b - a)
        if g < last.size:
            last_out[g] = xids[b - 1]
    return xids, last_out


def pending_add(tsock, table, new_sock, new):
    """(msock int64, merged CALL_DTYPE, old_pos, new_pos int64): every
    socket's calls_ after its sends, in socket order."""
    ns = np.asarray(new_sock).astype(np.int64)
    total = len(table) + len(new)
    msock = np.zeros(total, dtype=np.int64)
    merged = np.zeros(total, dtype=R.CALL_DTYPE)
    old_pos, new_pos = np.zeros(len(table), dtype=np.int64), np.zeros(len(new), dtype=np.int64)
    for g in socks_of(tsock, ns):
        lo, hi = run_of(tsock, g)
        a, b = run_of(ns, g)
        t, op, np_ = CS.merge(table["xid"][lo:hi], table["res"][lo:hi], new["xid"][a:b], new["res"][a:b])
        merged[lo + a:hi + b], msock[lo + a:hi + b] = t, g
        old_pos[lo:hi], new_pos[a:b] = np.asarray(op) + lo + a, np.asarray(np_) + lo + a
    return msock, merged, old_pos, new_pos


# --------------------------------------------------------------- recv_msg
def msg_socks(rows, row_sock, nrows: int) -> np.ndarray:
    """The socket of every message, -1 for a row that is no row."""
    rows = np.asarray(rows).astype(np.int64) & M32
    ok = rows < nrows
    safe = np.where(ok, rows, 0)
    s = safe if row_sock is None else (np.asarray(row_sock).astype(np.int64) & M32)[safe] if nrows else safe
    return np.where(ok, s, -1)


def match(stream: np.ndarray, offsets: np.ndarray, msock, socks, xids):
    """reply_model.match with every message looked up in the calls_ of its
    socket (msock[i], -1: no socket).  Returns (hdrs, call, reply_of)."""
    hdrs = O.rpc_headers(stream, offsets, None, client=True).copy()
    n = len(offsets) - 1
    calls_: dict[int, dict[int, int]] = {}
    for c, (g, x) in enumerate(zip(np.asarray(socks).astype(np.int64).tolist(), u32(xids).tolist())):
        assert x not in calls_.setdefault(g, {}), "duplicate (sock, xid)"
        calls_[g][x] = c
    call = np.full(n, -1, dtype=np.int64)
    reply_of = np.full(len(u32(xids)), -1, dtype=np.int64)
    for i in range(n):
        m0, m1 = int(offsets[i]), int(offsets[i + 1])
        if m1 > stream.size or m1 < m0 or m1 - m0 < 12 or m0 & 3:
            continue
        if RM.be_word(stream, m0 + 8) != RM.REPLY:
            continue
        mine = calls_.get(int(msock[i]), {}) if msock[i] >= 0 else {}
        c = mine.pop(RM.be_word(stream, m0 + 4), None)  # calls_.erase at the first reply
        if c is None:
            hdrs["action"][i] = A.RPCR_UNKNOWN_XID      # "ignoring reply to unknown call"
            continue
        call[i], reply_of[c] = c, i
    return hdrs, call, reply_of


def match_per_socket(stream: np.ndarray, offsets: np.ndarray, msock, socks, xids):
    """(action, call, reply_of) by reply_model.match itself, run once per
    socket on that socket's messages alone (copied out into a stream of their
    own) and its own xids."""
    n = len(offsets) - 1
    socks, x = np.asarray(socks).astype(np.int64), u32(xids)
    action = O.rpc_headers(stream, offsets, None, client=True)["action"].copy()
    call = np.full(n, -1, dtype=np.int64)
    reply_of = np.full(x.size, -1, dtype=np.int64)
    for g in socks_of(msock):
        mine = np.nonzero(np.asarray(msock) == g)[0]
        mycalls = np.nonzero(socks == g)[0] if g >= 0 else np.zeros(0, dtype=np.int64)
        pieces = [stream[int(offsets[i]):int(offsets[i + 1])] for i in mine]
        sub = np.concatenate(pieces + [np.zeros(0, np.uint8)])
        so = np.concatenate([[0], np.cumsum([p.size for p in pieces])]).astype(np.uint64)
        h, c, r = RM.match(sub, so, x[mycalls])
        action[mine] = h["action"]
        call[mine] = np.where(c >= 0, mycalls[np.clip(c, 0, None)] if mycalls.size else -1, -1)
        reply_of[mycalls] = np.where(r >= 0, mine[np.clip(r, 0, None)] if mine.size else -1, -1)
    return action, call, reply_of


# ------------------------------------------------------- stats and retire
def closed_of(closed, socks) -> np.ndarray:
    """abort_all_calls ran on the call's socket; a socket that is no socket
    counts as open."""
    closed, g = np.asarray(closed), np.asarray(socks).astype(np.int64)
    ok = (g >= 0) & (g < closed.size)
    return ok & (closed[np.where(ok, g, 0)] != 0 if closed.size else False)


def call_stats(hdrs: np.ndarray, reply_of, socks, closed) -> np.ndarray:
    """settle_model.call_stats, aborted or not by the call's own socket."""
    return np.where(closed_of(closed, socks), SM.call_stats(hdrs, reply_of, True), SM.call_stats(hdrs, reply_of, False))


def retire(socks, xids, res, reply_of, closed):
    """Every calls_ after the erases and the aborts, by settle_model.retire on
    one socket at a time.  Returns (tsock, table, old_of_new, inv) as
    SockCalls holds them: survivors renumbered in ascending old caller
    position."""
    socks, x = np.asarray(socks).astype(np.int64), u32(xids)
    r = np.broadcast_to(u32(res) if np.ndim(res) else np.uint32(res), x.shape)
    reply_of = np.asarray(reply_of).astype(np.int64)
    dead = closed_of(closed, socks)
    parts = []
    for g in socks_of(socks):
        mine = np.nonzero(socks == g)[0]
        gone = np.where(dead[mine], 0, reply_of[mine])  # abort_all_calls: calls_.clear()
        t, old, _ = SM.retire(x[mine], r[mine], gone)
        parts.append((g, t, mine[old]))
    old_of_new = np.sort(np.concatenate([p[2] for p in parts] + [np.zeros(0, np.int64)])).astype(np.int64)
    tsock = np.concatenate([np.full(len(p[1]), p[0], dtype=np.int64) for p in parts] + [np.zeros(0, np.int64)])
    table = np.concatenate([p[1] for p in parts] + [np.zeros(0, R.CALL_DTYPE)])
    # the table position of new call p: its (sock, xid) in the new table
    new_of_old = {int(c): p for p, c in enumerate(old_of_new)}
    inv = np.zeros(old_of_new.size, dtype=np.int64)
    at = 0
    for g, t, mine_old in parts:
        by_xid = {int(x[c]): c for c in mine_old}
        for k, e in enumerate(t):
            inv[new_of_old[int(by_xid[int(e["xid"])])]] = at + k
        at += len(t)
    return tsock, table, old_of_new, inv


def retire_arrays(tsock, table, reply_of_table, closed):
    """The three passes (settle_model.retire_arrays) with the keep rule "no
    reply and its socket open": (kept, kept_sock, kept_pos uint64, count)."""
    rt = np.asarray(reply_of_table).astype(np.uint64)
    rt = np.where(closed_of(closed, tsock), np.uint64(0), rt)
    kept, kept_pos, count, _ = SM.retire_arrays(table, rt)
    return kept, np.asarray(tsock)[rt == NO_CALL], kept_pos, count


# ------------------------------------------------------------- the cases
def _pending(rng, k: int) -> np.ndarray:
    return np.unique(rng.integers(1 << 32, size=k + 8, dtype=np.int64).astype(np.uint32))[:k]


def xid_cases():
    """(name, socks, xids, res of the pending calls in the caller's order,
    last [nsocks], call_sock [n]) for next_xids and pending_add."""
    rng = np.random.default_rng(88)
    out = []

    def case(name, per_sock: list, last, runs, extra_calls=()):
        socks = np.concatenate([np.full(len(p), g, dtype=np.int64) for g, p in enumerate(per_sock)] + [np.zeros(0, np.int64)])
        xids = np.concatenate([u32(p) for p in per_sock] + [np.zeros(0, np.uint32)])
        order = rng.permutation(xids.size)
        call_sock = np.concatenate([np.full(c, g, dtype=np.int64) for g, c in enumerate(runs)] + [np.asarray(extra_calls, dtype=np.int64)])
        out.append((name, socks[order], xids[order], rng.integers(61, size=xids.size).astype(np.uint32),
                    u32(last), call_sock))

    # runs of 0, 1, 63, 64, 65 and 257 calls a socket; empty sockets first, in the middle and last; the same xids
    # pending on neighbouring sockets; a last just below a pending block and one just below 2^32
    same = _pending(rng, 90)
    block = CS._run(5000, 40)
    case("runs", [same, same, _pending(rng, 300), np.zeros(0), block, same, np.concatenate([block, same]), _pending(rng, 7),
                  same], [0, 7, 0xFFFFFFC0, 3, 4999, int(same[10]) - 1, 4990, 0xFFFFFFFF, 1],
         [0, 1, 63, 0, 64, 65, 257, 0, 0])
    case("one_socket_all", [_pending(rng, 20), _pending(rng, 500), _pending(rng, 20)], [5, 0xFFFFFE00, 6], [0, 1000, 0])
    case("nsocks1", [_pending(rng, 300)], [0xFFFFFF80], [400])
    case("pending_0_after_wrap", [[0xFFFFFFFF, 0, 2]] * 4, [0xFFFFFFFD] * 4, [5, 5, 0, 5])
    case("wrap_in_one_run", [_pending(rng, 50), CS._run(0xFFFFFFF0, 40), _pending(rng, 50)], [10, 0xFFFFFF00, 20],
         [300, 300, 300])
    case("n0", [_pending(rng, 70), _pending(rng, 3)], [1, 2], [0, 0])
    case("ncalls0", [[], [], []], [0, 0xFFFFFFFE, 9], [65, 3, 64])
    case("all_empty", [[], []], [4, 5], [0, 0])
    return out


XID_CASES = xid_cases()

SIZES = SM.SIZES
CLOSED_MASKS = ("none", "all", "alternating", "across_tile", "lane0", "lane63")
ANSWERED = ("none", "all", "random")


def settle_socks(nc: int):
    """The socket of every TABLE entry of an nc-entry table, and nsocks:
    sockets of mixed sizes, among them socket 2 = the entries 250..262 (it
    spans the first tile boundary), socket 4 = the single entry 320 (lane 0 of
    its wave) and socket 6 = the single entry 383 (lane 63)."""
    j = np.arange(nc)
    s = np.select([j < 100, j < 250, j < 263, j < 320, j < 321, j < 383, j < 384], [0, 1, 2, 3, 4, 5, 6],
                  7 + (j - 384) // 97)
    return s.astype(np.int64), (int(s.max()) + 2 if nc else 3)  # the last socket has no call


def closed_mask(name: str, nsocks: int) -> np.ndarray:
    g = np.arange(nsocks)
    return {"none": g < 0, "all": g >= 0, "alternating": g % 2 == 1, "across_tile": g == 2, "lane0": g == 4,
            "lane63": g == 6}[name].astype(np.uint32) * np.uint32(0x01000000 if name == "lane0" else 1)


def settle_table(nc: int):
    """(tsock, table, nsocks) for the stats and retire cases: xids repeat from
    socket to socket."""
    tsock, nsocks = settle_socks(nc)
    rng = np.random.default_rng(500 + nc)
    table = np.zeros(nc, dtype=R.CALL_DTYPE)
    for g in socks_of(tsock):
        lo, hi = run_of(tsock, g)
        pool = np.unique(np.concatenate([[0, 1, 0xFFFFFFFF], rng.integers(1 << 20, size=2 * (hi - lo) + 8)])).astype(np.uint32)
        table["xid"][lo:hi] = np.sort(rng.permutation(pool)[:hi - lo])
    table["res"] = rng.integers(61, size=nc)
    return tsock, table, nsocks


def answered(name: str, nc: int) -> np.ndarray:
    """reply_of in table order (uint64), values that are no message number
    among the answered ones."""
    return SM.answered_values(SM.answered_mask(name, nc))


def call_stats_arrays(hdrs: np.ndarray, reply_of_table, tsock, closed) -> np.ndarray:
    """call_stats in array form, table order (for the large tables):
    rpc_call_stat(hdr) by masks instead of a walk."""
    rt = np.asarray(reply_of_table).astype(np.uint64)
    out = np.zeros(rt.size, dtype=SM.STAT)
    out["type"] = A.RPCS_GARBAGE_RES
    none = rt == NO_CALL
    out["type"][none] = np.where(closed_of(closed, tsock)[none], A.RPCS_NETWORK_ERROR, A.RPCS_PENDING)
    inb = ~none & (rt < np.uint64(len(hdrs)))
    h = hdrs[np.where(inb, rt, np.uint64(0)).astype(np.int64)] if len(hdrs) else np.zeros(rt.size, dtype=hdrs.dtype)
    a = h["action"]
    for action, ty, word in ((A.RPCR_OK, A.RPCS_ACCEPT_STAT, None), (A.RPCR_ACCEPT_STAT, A.RPCS_ACCEPT_STAT, A.RPC_W_STAT),
                             (A.RPCR_AUTH_STAT, A.RPCS_AUTH_STAT, A.RPC_W_WHY),
                             (A.RPCR_RPCVERS_MISMATCH, A.RPCS_RPCVERS_MISMATCH, None)):
        m = inb & (a == action)
        out["type"][m] = ty
        if word is not None:
            out["stat"][m] = h["w"][m, word]
    return out


# -------------------------------------------------------- the match cases
def reply_stream(xids, kinds=None):
    """Messages of 28 bytes: mark, xid, REPLY (or what `kinds` says: 0 a CALL,
    -1 a 4-byte message), MSG_ACCEPTED, verf, SUCCESS."""
    kinds = np.ones(len(xids), dtype=np.int64) if kinds is None else np.asarray(kinds)
    pieces = []
    for x, k in zip(xids, kinds):
        if k < 0:
            pieces.append(np.array([0x80000004, int(x)], dtype=">u4").view(np.uint8))
        elif k == 0:
            pieces.append(np.array([0x80000028, int(x), 0, 2, 1, 1, 1, 0, 0, 0, 0], dtype=">u4").view(np.uint8))
        else:
            pieces.append(np.array([0x80000018, int(x), 1, 0, 0, 0, 0], dtype=">u4").view(np.uint8))
    s = np.concatenate(pieces + [np.zeros(0, np.uint8)])
    o = np.concatenate([[0], np.cumsum([p.size for p in pieces])]).astype(np.uint64)
    return s, o


def match_case(name: str):
    """(socks, xids of the pending calls, stream, offsets, rows, row_sock,
    nrows) of the match cases of the GPU tests."""
    rng = np.random.default_rng(31)
    if name == "xid1_on_three":
        # xid 1 pending on sockets 0, 2 and 5; socket 3 has another call, socket 4 none
        socks, xids = np.array([0, 2, 5, 3, 2]), np.array([1, 1, 1, 9, 7])
        # replies: on a socket with no calls (4), on a wrong socket (3), ahead of the right one (2: twice, the
        # second is late), on 0 and 5, and an xid pending elsewhere only (7 on socket 0)
        rows = np.array([4, 3, 2, 2, 0, 5, 0, 1])
        return socks, xids, *reply_stream([1, 1, 1, 1, 1, 1, 7, 1]), rows, None, 6
    if name == "wrong_first":
        # the wrong-socket reply has the lower message index: it must not win the call
        socks, xids = np.array([1, 1, 0]), np.array([5, 6, 6])
        return socks, xids, *reply_stream([5, 5, 6, 6]), np.array([0, 1, 1, 0]), None, 2
    if name == "row_map":
        # rows of the round mapped to sockets; row 3 is past nrows, and so is 0xFFFFFFFF
        socks, xids = np.array([7, 7, 2, 2, 0]), np.array([1, 2, 1, 2, 1])
        rows = np.array([0, 1, 2, 3, 0xFFFFFFFF, 1, 0, 2])
        return socks, xids, *reply_stream([1, 1, 1, 1, 1, 2, 2, 2]), rows, np.array([7, 2, 0]), 3
    assert name in ("dups_257", "mixed_257")
    # 257 messages over 6 sockets; xids 0..19 on every socket; duplicates 64 and more messages apart
    nsocks, n = 6, 257
    socks, xids = np.repeat(np.arange(nsocks), 20), np.tile(np.arange(20), nsocks)
    keep = rng.random(socks.size) < 0.8
    socks, xids = socks[keep], xids[keep]
    rows = rng.integers(nsocks + 1, size=n)
    mx = rng.integers(22, size=n)
    mx[64:128], rows[64:128] = mx[:64], rows[:64]      # the same (row, xid) one wave later
    mx[200:257], rows[200:257] = mx[3:60], rows[3:60]  # and across three
    kinds = np.ones(n, dtype=np.int64)
    if name == "mixed_257":
        kinds = rng.choice([1, 1, 1, 0, -1], size=n)
    order = rng.permutation(socks.size)
    return socks[order], xids[order], *reply_stream(mx, kinds), rows, None, nsocks


MATCH_CASES = ("xid1_on_three", "wrong_first", "row_map", "dups_257", "mixed_257")
