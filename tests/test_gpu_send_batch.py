"""GPU: xdrg_rpc_send_batch against the host model (tests/send_model.py), bit
for bit: stream, offsets, count, conn_of, origin, pos, every field of every
xdrg_rpc_wqueue record and counts; then the receive side, which is pinned to
the reference, as the second witness: what is queued for a connection, framed
by xdrg_rpc_recv_batch, is exactly the messages routed to it, in order."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD

from xdrpp_amd import _abi as A
from xdrpp_amd import marshal as M
from xdrpp_amd import rpc as R
import recv_model as RM
import send_model as SM

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64  # canary elements either side of an output
FILL = {torch.uint8: CANARY, torch.int32: 0x25A5A5A5, torch.int64: 0x25A5A5A5A5A5A5A5}
TILE = SM.SORT_TILE


def guarded(n: int, dtype, dev):
    """(whole, view): n elements with PAD canary elements either side."""
    whole = torch.full((n + 2 * PAD,), FILL[dtype], dtype=dtype, device=dev)
    return whole, whole[PAD:PAD + n]


def intact(whole: torch.Tensor, n: int) -> bool:
    fill = FILL[whole.dtype]
    return bool((whole[:PAD] == fill).all().item() and (whole[PAD + n:] == fill).all().item())


def as_i64(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy())


def device_sources(dev, sources):
    out = []
    for s in sources:
        conn = s["conn"] if isinstance(s["conn"], (int, np.integer)) else \
            torch.from_numpy(np.ascontiguousarray(s["conn"], dtype=np.uint32).view(np.int32).copy()).to(dev)
        count = None if s["count"] is None else as_i64(np.array([s["count"]], dtype=np.uint64)).to(dev)
        out.append(R.SendSource(torch.from_numpy(np.ascontiguousarray(s["bytes"])).to(dev), as_i64(s["offsets"]).to(dev),
                                conn, count, s["cap"]))
    return out


def run(dev, sources, nconns, closed=None, cap=None, with_pos=True, with_counts=True, on_device=False):
    """One call through the launch_ mirror with canaries round every output.
    Returns a dict of numpy results (on_device: the queues stay a tensor)."""
    srcs = device_sources(dev, sources)
    entries = sum(s["cap"] for s in sources)
    cap = sum(s["bytes"].size for s in sources) if cap is None else cap
    d_closed = None if closed is None else torch.from_numpy(np.asarray(closed, dtype=np.int32)).to(dev)
    out_w, out = guarded(cap, torch.uint8, dev)
    offs_w, offs = guarded(entries + 1, torch.int64, dev)
    cof_w, cof = guarded(entries, torch.int32, dev)
    org_w, org = guarded(entries, torch.int64, dev)
    pos_w, pos = guarded(entries, torch.int64, dev)
    q_w, q = guarded(4 * nconns, torch.int64, dev)
    cnts_w, cnts = guarded(4, torch.int64, dev)
    cnt_w, cnt = guarded(1, torch.int64, dev)
    ws = torch.empty(max(A.lib().xdrg_rpc_send_batch_workspace_size(entries, nconns), 16), dtype=torch.uint8,
                     device=dev)
    st = M.Status(dev)
    s = torch.cuda.current_stream().cuda_stream
    st.init(s)
    R.launch_send_batch(srcs, nconns, d_closed, out, offs, cnt, cof, org, pos if with_pos else None, q,
                        cnts if with_counts else None, st, ws, s)
    e = st.read(s)
    for w, k in ((out_w, cap), (offs_w, entries + 1), (cof_w, entries), (org_w, entries), (pos_w, entries),
                 (q_w, 4 * nconns), (cnts_w, 4), (cnt_w, 1)):
        assert intact(w, k)
    if not with_pos:
        assert (pos == FILL[torch.int64]).all().item()
    if not with_counts:
        assert (cnts == FILL[torch.int64]).all().item()
    n = int(cnt.item())
    assert 0 <= n <= entries
    return {"stream": out.cpu().numpy(), "offsets": offs.cpu().numpy().view(np.uint64), "count": n,
            "conn_of": cof.cpu().numpy().view(np.uint32), "origin": org.cpu().numpy().view(np.uint64),
            "pos": pos.cpu().numpy(), "queues": q if on_device else R.wqueues_numpy(q),
            "counts": tuple(cnts.tolist()), "code": int(e.code), "record": int(e.record),
            "total_bytes": int(e.total_bytes)}


def same(got, want, with_pos=True, with_counts=True):
    assert got["code"] == 0, (got["code"], got["record"])
    m = want["count"]
    assert got["count"] == m and got["total_bytes"] == want["total_bytes"] == want["stream"].size
    assert np.array_equal(got["offsets"][:m + 1], want["offsets"])
    assert np.array_equal(got["conn_of"][:m], want["conn_of"])
    assert np.array_equal(got["origin"][:m], want["origin"])
    if with_pos:
        assert np.array_equal(got["pos"], want["pos"]), np.nonzero(got["pos"] != want["pos"])[0][:8]
    if with_counts:
        assert got["counts"] == want["counts"]
    if isinstance(got["queues"], torch.Tensor):
        ref = torch.from_numpy(want["queues"].view(np.int64).copy()).to(got["queues"].device)
        assert torch.equal(got["queues"], ref)
    else:
        assert got["queues"].tobytes() == want["queues"].tobytes(), \
            [(i, a, b) for i, (a, b) in enumerate(zip(got["queues"].tolist(), want["queues"].tolist())) if a != b][:5]
    assert got["stream"][:want["stream"].size].tobytes() == want["stream"].tobytes()


def check(dev, sources, nconns, closed=None, **kw):
    want = SM.send_batch(sources, nconns, closed)
    got = run(dev, sources, nconns, closed, **kw)
    same(got, want, kw.get("with_pos", True), kw.get("with_counts", True))
    return got, want


def tagged(seed, conn, bodies=None):
    """One source of len(conn) messages, message i tagged i (bodies of 1..6
    words by default, so every message is distinct)."""
    rng = np.random.default_rng(seed)
    n = len(conn)
    bodies = 4 * rng.integers(1, 7, n) if bodies is None else bodies
    return SM.source([SM.message(rng, int(b), tag=i) for i, b in enumerate(bodies)], conn)


# ------------------------------------------------------- 1. entry counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1])
def test_entry_counts(dev, n):
    """Lane, wave, 256-entry tile and sort tile edges, seven connections in a
    seeded order."""
    assert TILE == 2048
    rng = np.random.default_rng(n)
    got, want = check(dev, [tagged(n, rng.integers(0, 7, n))], 7)
    assert want["count"] == n and (n < 200 or (np.diff(want["keys"]) < 0).any())


def test_no_source_at_all(dev):
    got, want = check(dev, [], 5)
    assert got["count"] == 0 and got["queues"].tolist() == [(0, 0, 0, 0)] * 5 and got["counts"] == (0, 0, 0, 0)


@pytest.mark.parametrize("n", [SM.TILE * SM.SCAN_LANES + 1, TILE * SM.SCAN_LANES + 1])
def test_scan_carry(dev, n):
    """256 * 1024 + 1 entries: the second round of k_tile_scan (and, with 256
    counters a sort tile, the ninth round of the pass scan); 2048 * 1024 + 1:
    1025 sort tiles.  Bare marks keep the stream small; 300 connections take two
    passes."""
    rng = np.random.default_rng(5)
    conn = rng.integers(0, 300, n)
    check(dev, [SM.marks_source(n, conn)], 300)


# -------------------------------------------------- 2. connection counts
@pytest.mark.parametrize("nconns", [1, 2, 255, 256, 65535, 65536])
def test_connection_counts(dev, nconns):
    """Either side of every added pass: the highest connection and the
    sentinel nconns differ from the rest in the top digit."""
    rng = np.random.default_rng(nconns)
    n = 3000
    conn = rng.integers(0, nconns, n)
    conn[rng.integers(0, n, 40)] = nconns - 1
    conn[rng.integers(0, n, 40)] = 0
    src = tagged(nconns, conn)
    src["conn"][[7, 900, 2999]] = nconns            # unusable: they sort with the sentinel
    check(dev, [src], nconns)


def test_one_connection_in_order_and_not(dev):
    """One connection: every key is 0 or the sentinel 1.  All queued is in
    order; an empty entry before a queued one is a descent."""
    src = tagged(1, np.zeros(500, dtype=np.uint32))
    got, want = check(dev, [src], 1)
    assert (np.diff(want["keys"]) >= 0).all() and np.array_equal(got["pos"], np.arange(500))
    holes = SM.source([m if i % 5 else np.zeros(0, np.uint8) for i, m in enumerate(np.split(src["bytes"],
                       src["offsets"][1:-1].astype(int)))], 0)
    got, want = check(dev, [holes], 1)
    assert (np.diff(want["keys"]) < 0).any() and got["count"] == 400


def test_sixteen_million_connections(dev):
    """2^24 + 1 connections, 1,000 messages: the fourth pass.  The queue
    records are compared on the device."""
    nconns = (1 << 24) + 1
    rng = np.random.default_rng(24)
    conn = rng.integers(0, nconns, 1000)
    conn[:4] = [nconns - 1, 1 << 24, 0, nconns - 1]
    check(dev, [tagged(24, conn)], nconns, on_device=True)


# ------------------------------------------------------- 3. key patterns
def pattern(name, n, nconns):
    i = np.arange(n)
    if name == "all_equal":
        return np.full(n, nconns // 3)
    if name == "ascending":
        return i * nconns // n
    if name == "descending":
        return (n - 1 - i) * nconns // n
    if name == "mod":
        return i % nconns
    if name == "random":
        return np.random.default_rng(3).integers(0, nconns, n)
    if name == "top_digit":
        return ((i * 7) % 5 << 16) | 0x1234
    assert name == "bottom_digit"
    return 0x30100 | ((i * 37) % 256)


@pytest.mark.parametrize("name", ["all_equal", "ascending", "descending", "mod", "random", "top_digit",
                                  "bottom_digit"])
def test_key_patterns(dev, name):
    """5,000 messages over 330,000 connections (three passes); i mod nconns
    over 300, or it would ascend."""
    n, nconns = 5000, 300 if name == "mod" else 330000
    conn = pattern(name, n, nconns)
    assert conn.max() < nconns
    got, want = check(dev, [tagged(8, conn)], nconns)
    inorder = bool((np.diff(want["keys"]) >= 0).all())
    assert inorder == (name in ("all_equal", "ascending"))
    if inorder:  # the identity: what the passes would have had to produce, without them
        assert np.array_equal(got["pos"], np.arange(n)) and np.array_equal(got["origin"][:n], np.arange(n))


def test_ascending_with_a_late_descent(dev):
    """In order but for the very last pair, and but for one pair that
    straddles two 256-entry tiles: neither may take the fast path."""
    n, nconns = 3 * TILE, 1000
    for at in (n - 1, 512):
        conn = np.arange(n) * nconns // n
        conn[at] = conn[at - 1] - 1
        got, want = check(dev, [tagged(at, conn)], nconns)
        assert got["pos"][at] < at


# ---------------------------------------------------------- 4. stability
def test_stability_across_lane_wave_and_tile_edges(dev):
    """Connection 5's messages, each with its own body, stand at the last and
    first lanes of waves, of 256-entry tiles and of sort tiles, between other
    connections' messages on both sides of it."""
    n = 2 * TILE + 300
    rng = np.random.default_rng(17)
    conn = rng.integers(0, 11, n)
    conn[conn == 5] = 6
    mine = sorted({k + d for k in (64, 128, 256, 512, TILE - 64, TILE, 2 * TILE) for d in (-2, -1, 0, 1)} | {0, n - 1})
    conn[mine] = 5
    got, want = check(dev, [tagged(17, conn)], 11)
    q = got["queues"][5]
    first, msgs = int(q["first"]), int(q["msgs"])
    assert msgs == len(mine) and got["origin"][first:first + msgs].tolist() == mine
    tags = [int.from_bytes(got["stream"][int(o) + 4:int(o) + 8].tobytes(), "big")
            for o in got["offsets"][first:first + msgs]]
    assert tags == mine


# ----------------------------------------------------- 5. several sources
def test_two_sources_alternate_on_the_same_connections(dev):
    n = 700
    conn = np.arange(n) % 9
    a, b = tagged(1, conn), tagged(2, conn[::-1].copy())
    got, want = check(dev, [a, b], 9)
    for c in range(9):  # source 0 first on every connection, each source in entry order
        q = got["queues"][c]
        org = got["origin"][int(q["first"]):int(q["first"] + q["msgs"])]
        assert (np.diff(org.astype(np.int64)) > 0).all() and (org >> 32).tolist() == sorted((org >> 32).tolist())
        assert set((org >> 32).tolist()) == {0, 1}


def test_a_source_for_one_connection_and_a_device_count(dev):
    """d_conn NULL: the whole stream goes to `conn`.  *d_count below count_cap:
    the entries past it are not used (d_pos -2, not counted); above it:
    count_cap holds."""
    conn = np.arange(300) % 4
    a = tagged(3, conn)
    b = tagged(4, np.zeros(100))
    b["conn"] = 2
    c = tagged(5, conn[:200] + 1)
    c["count"] = 130
    d = tagged(6, conn[:70])
    d["count"] = (1 << 40) + 3
    e = tagged(7, np.zeros(5))
    e["conn"] = 9                                   # a connection that is not there
    got, want = check(dev, [a, b, c, d, e], 5)
    assert (got["pos"][400 + 130:600] == SM.EMPTY).all() and (got["pos"][400:400 + 130] >= 0).all()
    assert got["counts"] == (300 + 100 + 130 + 70, 0, 0, 5) and (got["pos"][-5:] == SM.UNUSABLE).all()
    for kw in ({"with_pos": False}, {"with_counts": False}):
        check(dev, [a, b, c, d, e], 5, **kw)


# -------------------------------------------- 6. the non-queued outcomes
GOOD_N = 200


def good_part(lo, hi):
    conn = (np.arange(GOOD_N) * 5) % 7
    conn[conn == 3] = 4                             # connection 3 takes nothing: it is the closed one
    whole = tagged(60, conn)
    msgs = np.split(whole["bytes"], whole["offsets"][1:-1].astype(int))
    return SM.source(msgs[lo:hi], conn[lo:hi])


@pytest.fixture(scope="module")
def good_alone(dev):
    return check(dev, [good_part(0, GOOD_N)], 7, closed=[0, 0, 0, 1, 0, 0, 0])


def odd_one(kind):
    rng = np.random.default_rng(1)
    m = SM.message(rng, 24, tag=77)
    s = SM.source([m], [2])
    if kind == "empty":
        s = SM.source([np.zeros(0, np.uint8)], [2])
    elif kind == "end_before_begin":
        s["offsets"] = np.array([28, 0], dtype=np.uint64)
    elif kind == "end_past_the_stream":
        s["offsets"] = np.array([0, 32], dtype=np.uint64)
    elif kind == "offset_not_aligned":
        s = SM.source([np.concatenate([m[:2], m])], [2])
        s["offsets"] = np.array([2, 30], dtype=np.uint64)
    elif kind == "length_not_aligned":
        s["offsets"] = np.array([0, 26], dtype=np.uint64)
    elif kind == "below_a_mark":
        s["offsets"] = np.array([0, 2], dtype=np.uint64)
    elif kind == "mark_without_last_bit":
        s["bytes"][0] = 0
    elif kind == "mark_of_another_length":
        s["bytes"][3] = 20
    elif kind == "connection_past_nconns":
        s["conn"] = np.array([7], dtype=np.uint32)
    else:
        assert kind == "closed"
        s["conn"] = np.array([3], dtype=np.uint32)
    return s


ODD = ["empty", "end_before_begin", "end_past_the_stream", "offset_not_aligned", "length_not_aligned",
       "below_a_mark", "mark_without_last_bit", "mark_of_another_length", "connection_past_nconns", "closed"]


@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("kind", ODD)
def test_one_odd_entry_changes_nothing_else(dev, good_alone, kind, lane):
    base, _ = good_alone
    at = 64 + lane
    got, want = check(dev, [good_part(0, at), odd_one(kind), good_part(at, GOOD_N)], 7, closed=[0, 0, 0, 1, 0, 0, 0])
    code = {"empty": SM.EMPTY, "closed": SM.DROPPED}.get(kind, SM.UNUSABLE)
    assert got["pos"][at] == code
    assert got["counts"] == (GOOD_N, int(code == SM.DROPPED), int(code == SM.EMPTY), int(code == SM.UNUSABLE))
    assert np.array_equal(np.delete(got["pos"], at), base["pos"])
    m = GOOD_N
    assert got["count"] == base["count"] == m and got["queues"].tobytes() == base["queues"].tobytes()
    assert np.array_equal(got["offsets"][:m + 1], base["offsets"][:m + 1])
    assert got["stream"][:base["total_bytes"]].tobytes() == base["stream"][:base["total_bytes"]].tobytes()
    assert np.array_equal(got["conn_of"][:m], base["conn_of"][:m])


# -------------------------------------------------------- 7. message sizes
def test_message_sizes(dev):
    """A bare mark, 8, 16,380, 16,384 bytes, 20 KiB and 1 MiB, with small
    neighbours in the same wave, out of order over five connections."""
    sizes = [4, 8, 12, 16380, 8, 16384, 4, 20 * 1024, 24, 1 << 20, 8, 4, 16380, 1 << 20, 12, 16384] + [8, 4, 40] * 10
    rng = np.random.default_rng(7)
    conn = rng.integers(0, 5, len(sizes))
    got, want = check(dev, [tagged(7, conn, bodies=[s - 4 for s in sizes])], 5)
    assert want["count"] == len(sizes) and want["total_bytes"] == sum(sizes)


# ------------------------------------------------------------ 8. capacity
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_capacity(dev, where):
    src = tagged(9, np.random.default_rng(9).integers(0, 6, 700))
    full = SM.send_batch([src], 6)
    m = full["count"]
    j = {"first": 0, "middle": 333, "last": m - 1}[where]
    cap = int(full["offsets"][j + 1]) - 4               # four bytes short of position j's end
    want = SM.send_batch([src], 6, capacity=cap)
    assert (want["code"], want["record"]) == (A.ERR_OVERFLOW_PUT, j)
    got = run(dev, [src], 6, cap=cap)                   # the canaries round d_out are run()'s
    assert (got["code"], got["record"]) == (A.ERR_OVERFLOW_PUT, j)
    upto = int(full["offsets"][j])
    assert got["stream"][:upto].tobytes() == full["stream"][:upto].tobytes() == want["stream"].tobytes()
    assert (got["stream"][upto:] == CANARY).all()       # nothing of the message that does not fit, nor after it
    assert got["count"] == m and got["total_bytes"] == full["total_bytes"]
    assert np.array_equal(got["offsets"][:m + 1], full["offsets"]) and np.array_equal(got["pos"], full["pos"])
    assert got["queues"].tobytes() == full["queues"].tobytes() and got["counts"] == full["counts"]
    same(run(dev, [src], 6, cap=full["total_bytes"]), full)  # exactly enough is no error


# ------------------------------------------------- 9. device arrays that lie
@pytest.mark.parametrize("lie", ["descending_offsets", "ends_past_the_stream", "connections", "count_above_cap",
                                 "everything"])
def test_device_arrays_that_lie(dev, lie):
    """Whatever the device arrays hold, nothing outside the inputs is read and
    nothing outside the outputs written: the call returns what the contract
    says of such entries, and the canaries round every output hold (run()).
    The streams end at their last byte, so a read past one leaves the
    allocation's used part."""
    rng = np.random.default_rng(21)
    n = 1000
    a, b = tagged(21, rng.integers(0, 12, n)), tagged(22, rng.integers(0, 12, n))
    if lie in ("descending_offsets", "everything"):
        a["offsets"] = a["offsets"][::-1].copy()
        b["offsets"][100:200] = b["offsets"][100:200][::-1].copy()
    if lie in ("ends_past_the_stream", "everything"):
        b["offsets"][-1] = b["bytes"].size + 4
        b["offsets"][500] = 1 << 63
        b["offsets"][700] = (1 << 64) - 4
    if lie in ("connections", "everything"):
        a["conn"][::3] = 0xffffffff
        b["conn"][5::7] = 12
        b["conn"][6::7] = 1 << 31
    if lie in ("count_above_cap", "everything"):
        a["count"], b["count"] = (1 << 64) - 1, n + 1
    got, want = check(dev, [a, b], 12, closed=[0] * 11 + [1])
    assert want["counts"][3] > 0 or lie == "count_above_cap"


# ---------------------------------------------------------- 10. round trip
@pytest.mark.parametrize("seed", [31, 32])
def test_round_trip_through_the_receive_side(dev, seed):
    """Every connection's range of the queued stream, handed to
    xdrg_rpc_recv_batch as that connection's segment, delivers exactly the
    messages routed to it, in putmsg order."""
    rng = np.random.default_rng(seed)
    nconns, n = 41, 1500
    conn = [rng.integers(0, nconns, n), rng.integers(0, nconns, n)]
    for c in conn:
        c[c == 13] = 14                              # one connection with nothing to send
    parts = [tagged(seed + k, conn[k], bodies=4 * rng.integers(0, 30, n)) for k in range(2)]
    q = R.send_batch(device_sources(dev, parts), nconns)
    want = SM.send_batch(parts, nconns)
    assert q.count == want["count"] == 2 * n and q.counts == want["counts"]
    assert q.stream.cpu().numpy().tobytes() == want["stream"].tobytes()
    assert np.array_equal(q.ranges(), np.stack([want["queues"]["begin"], want["queues"]["begin"] +
                                                want["queues"]["len"]], axis=1).astype(np.int64))
    segs = np.zeros(nconns, dtype=A.CONN_IN_DTYPE)
    segs["begin"], segs["len"] = q.queues_numpy()["begin"], q.queues_numpy()["len"]
    got = R.recv_batch(q.stream, segs, rpc_sock=False)
    conns = got.conns_numpy()
    assert (conns["state"] == RM.OPEN).all() and (conns["need"] == 0).all()
    assert np.array_equal(conns["msgs"], q.queues_numpy()["msgs"]) and np.array_equal(conns["consumed"], segs["len"])
    assert got.count == q.count and torch.equal(got.offsets, q.offsets) and torch.equal(got.conn_of, q.conn_of)
    assert torch.equal(got.stream, q.stream)
    # and against the routing itself, message by message
    msgs = [np.split(p["bytes"], p["offsets"][1:-1].astype(int)) for p in parts]
    st, offs = got.stream.cpu().numpy(), got.offsets.cpu().numpy()
    for c in range(nconns):
        routed = [msgs[k][i].tobytes() for k in range(2) for i in np.nonzero(conn[k] == c)[0]]
        f, k = int(conns["first"][c]), int(conns["msgs"][c])
        assert [st[int(offs[j]):int(offs[j + 1])].tobytes() for j in range(f, f + k)] == routed, c


def test_calls_in_application_order(dev):
    """socks_call_batch_any_order against socks_call_batch on the same calls
    sorted by hand: the same stream, xids and pending table."""
    rng = np.random.default_rng(44)
    n, nsocks = 300, 6
    socks = rng.integers(0, nsocks, n)
    order = np.argsort(socks, kind="stable")
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    halves = [np.nonzero(np.arange(n) % 3 == r)[0] for r in range(3)]

    def sources(renumber):
        return [R.arg_source((7, 1, r), 10 + r, torch.from_numpy(renumber(h)).to(dev)) for r, h in enumerate(halves)]

    def fresh():
        return R.SockCalls([0, 3, 3], [1, 1, 2], [0, 0, 0], nsocks, dev, last=[1, 0, 0, 2, 0, 9])

    st, offs, xids, p2, ranges, got_order = R.socks_call_batch_any_order(fresh(), socks, sources(lambda h: h))
    st0, offs0, xids0, p20, ranges0 = R.socks_call_batch(fresh(), socks[order], sources(lambda h: inv[h]))
    assert torch.equal(st, st0) and torch.equal(offs, offs0) and np.array_equal(ranges, ranges0)
    assert np.array_equal(got_order.cpu().numpy(), order)
    assert np.array_equal(xids.cpu().numpy()[order], xids0.cpu().numpy())
    assert torch.equal(p2.table, p20.table) and torch.equal(p2.sock, p20.sock) and torch.equal(p2.last, p20.last)
    assert torch.equal(p2.inv[:3], p20.inv[:3]) and torch.equal(p2.inv[3:][torch.from_numpy(order).to(dev)], p20.inv[3:])
    with pytest.raises(ValueError, match="socket order"):
        R.socks_call_batch(fresh(), socks, sources(lambda h: h))     # the contract of the ordered call stands
    # the other recipe: one xid space, call_batch in caller order, then send_batch routes the stream
    pend = R.PendingCalls([], [], dev)
    cst, coffs, cx, _ = R.call_batch(pend, sources(lambda h: h), n)[:4]
    q = R.send_batch([(cst, coffs, socks)], nsocks)
    assert q.count == n and np.array_equal(q.origin.cpu().numpy(), order) and \
        np.array_equal(q.conn_of.cpu().numpy(), socks[order])


# ---------------------------------------------------------- 11. end to end
def g(name, dtype=np.uint8):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


NC, ROUNDS = 37, 5
DROPS = (A.RPC_DROP_MALFORMED, A.RPC_DROP_NONCALL)


def partial_writes(tx: R.Sender, rng, wire, final: bool):
    """Seeded writev results for every connection with something queued: a
    part of what iov() offers, everything, or EAGAIN; at the end whatever is
    left."""
    for c in range(NC):
        while tx.pending(c):
            v = tx.iov(c)
            offered = sum(len(b) for b in v)
            kind = int(rng.integers(0, 4))
            if kind == 0 and not final:
                break                                # EAGAIN: try again next round
            n = offered if kind == 1 or final else int(rng.integers(1, offered + 1))
            wire[c] += b"".join(bytes(b) for b in v)[:n]
            tx.wrote(c, n)
            if not final and kind == 2:
                break


def test_server_and_client_on_the_same_sockets(dev):
    """rpccall_1024.stream dealt to 37 connections and received in 5 rounds
    (as test_gpu_recv_batch.py does).  The service is asynchronous: half of a
    round's calls are answered at once, the rest shuffled in a later round,
    so a round sends the replies of several rounds' calls, as separate
    sources, plus calls of its own for the same connections.  Every round goes
    through send_batch and Sender with seeded partial writes.  What each
    connection finally wrote, framed by a client-side recv_batch and matched
    by socks_match_replies, answers every call exactly once, and carries the
    peer's own calls in order."""
    stream = g("rpccall_1024.stream")
    ref = g("rpccall_1024.hdrs").view(R.HDR_DTYPE)
    procs = g("rpc_procs.bin", "<u4").reshape(-1, 4)
    frames, consumed, _, state = RM.frame(stream)
    assert len(frames) == 1024 and consumed == stream.size
    whole = [stream[p:p + b] for p, b, _ in frames]
    dealt = [list(range(c, 1024, NC)) for c in range(NC)]
    data = [np.concatenate([whole[i] for i in d]) for d in dealt]
    rng = np.random.default_rng(37)
    cuts = [np.sort(rng.integers(0, x.size + 1, ROUNDS - 1)).tolist() for x in data]
    rx, tx = R.Receiver(), R.Sender()
    wire = [b"" for _ in range(NC)]
    owed = []                                        # (hdrs, conn of every message, withheld message numbers)
    own_calls = [[] for _ in range(NC)]
    sent_sources = 0
    for r in range(ROUNDS + 1):                      # one more round, to answer what the last one withheld
        sources = []
        if r < ROUNDS:
            for c, x in enumerate(data):
                lo = cuts[c][r - 1] if r else 0
                hi = cuts[c][r] if r < ROUNDS - 1 else x.size
                rx.feed(c, x[lo:hi].tobytes())
            buf, segs = rx.batch(pin=False)
            ids = torch.tensor(rx.ids, dtype=torch.int32, device=dev)
            got = R.recv_batch(buf.to(dev), segs, rpc_sock=False)
            rx.advance(got.conns_numpy())
        late, owed = owed, []
        for hd, conn, idx in late:                   # completion order: shuffled
            replies, ro = R.reply_batch(hd, [R.ResultSource(torch.from_numpy(rng.permutation(idx)).to(dev))])
            assert int((ro[1:] > ro[:-1]).sum().item()) == idx.size
            sources.append((replies, ro, conn))
        if r < ROUNDS and got.count:
            hd = R.dispatch(got.stream, got.offsets, procs)
            conn = ids[got.conn_of.to(torch.int64)]
            served = np.nonzero(R.hdrs_numpy(hd)["action"] == A.RPC_DISPATCH)[0]
            now = rng.random(served.size) < 0.5
            replies, ro = R.reply_batch(hd, [R.ResultSource(torch.from_numpy(served[now]).to(dev))])
            sources.append((replies, ro, conn))      # error replies, half of the answers, holes for the rest
            if (~now).any():                         # the same headers with everything else struck out
                h = R.hdrs_numpy(hd).copy()
                h["action"][np.setdiff1d(np.arange(h.size), served[~now])] = A.RPC_DROP_NONCALL
                owed.append((torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev), conn, served[~now]))
        k = int(rng.integers(20, 60))                # the peer's own calls, for the same connections
        mine = [RM.message(rng, 4 * int(rng.integers(2, 9)), word1=0) for _ in range(k)]
        to = rng.integers(0, NC, k)
        for m, c in zip(mine, to):
            own_calls[c].append(m.tobytes())
        own = SM.source(mine, to)
        sources.append(device_sources(dev, [own])[0])
        sent_sources = max(sent_sources, len(sources))
        q = R.send_batch(sources, NC, tx.closed(NC))
        assert q.counts[1] == q.counts[3] == 0
        tx.queue(q)
        partial_writes(tx, rng, wire, final=r == ROUNDS)
    assert not rx.closed and sent_sources >= 3 and all(tx.pending(c) == 0 for c in range(NC))
    # the client: every call that is owed a reply, on the socket it went out on
    owing = [i for i in range(1024) if ref["action"][i] not in DROPS]
    sock_of = np.empty(1024, dtype=np.int64)
    for c, d in enumerate(dealt):
        sock_of[d] = c
    pending = R.SockCalls(sock_of[owing], ref["xid"][owing], np.zeros(len(owing), np.uint32), NC, dev)
    buf, segs = RM.pack([np.frombuffer(w, dtype=np.uint8) for w in wire])
    back = R.recv_batch(torch.from_numpy(buf).to(dev), segs)
    assert (back.conns_numpy()["state"] == RM.OPEN).all() and (back.conns_numpy()["need"] == 0).all()
    kind = back.kind.cpu().numpy()
    assert int((kind == 1).sum()) == len(owing)      # as many replies as calls that are owed one
    hdrs, call, reply_of = R.socks_match_replies(back.stream, back.offsets, back.conn_of, pending)
    call = call.cpu().numpy()
    assert (call[kind == 1] >= 0).all() and sorted(call[kind == 1].tolist()) == list(range(len(owing)))
    assert (reply_of.cpu().numpy() >= 0).all()       # every call exactly once
    st, offs, cof = back.stream.cpu().numpy(), back.offsets.cpu().numpy(), back.conn_of.cpu().numpy()
    for c in range(NC):
        got_calls = [st[int(offs[j]):int(offs[j + 1])].tobytes() for j in np.nonzero((cof == c) & (kind == 0))[0]]
        assert got_calls == own_calls[c], c


# -------------------------------------------------------- 12. graph capture
def test_graph_capture(dev):
    """One capture of recv_batch -> dispatch -> reply_batch -> send_batch,
    replayed over three other contents: the replies routed back to the
    connections the calls came in on (in connection order: the passes stand
    aside) and to seeded other ones (they do not).  The launch sequence is the
    same either way, or the replay could not follow."""
    stream = g("rpccall_1024.stream")
    ref = g("rpccall_1024.hdrs").view(R.HDR_DTYPE)
    procs_np = g("rpc_procs.bin", "<u4").reshape(-1, 4)
    frames, _, _, _ = RM.frame(stream)
    keep = [i for i in range(1024) if ref["action"][i] not in DROPS]   # every message gets a reply
    n = len(keep)
    msgs = [stream[frames[i][0]:frames[i][0] + frames[i][1]] for i in keep]

    def contents(seed):
        rng = np.random.default_rng(seed)
        order = rng.permutation(n)
        buf, segs = RM.pack([np.concatenate([msgs[i] for i in order[c::NC]]) for c in range(NC)])
        conn_of = RM.recv_batch(buf, segs, RM.MAXLEN, False)[2]
        route = conn_of if seed % 2 else rng.integers(0, NC, n)
        return buf, segs, route.astype(np.int32)

    size = max(contents(s)[0].size for s in range(4))
    L = A.lib()
    d_buf = torch.zeros(size, dtype=torch.uint8, device=dev)
    d_segs = torch.zeros(2 * NC, dtype=torch.int64, device=dev)
    route = torch.zeros(n, dtype=torch.int32, device=dev)
    max_msgs = size // 4
    out = torch.empty(size, dtype=torch.uint8, device=dev)
    offs = torch.empty(max_msgs + 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    cof = torch.empty(max_msgs, dtype=torch.int32, device=dev)
    conns = torch.empty(4 * NC, dtype=torch.int64, device=dev)
    hdrs = torch.empty(n * A.RPC_HDR_BYTES, dtype=torch.uint8, device=dev)
    procs = torch.from_numpy(np.ascontiguousarray(procs_np, dtype=np.uint32).view(np.int32)).to(dev)
    answers = R.ResultSource(torch.arange(n, dtype=torch.int64, device=dev))   # void results: whoever is served
    replies = torch.empty(36 * n + 28 * n, dtype=torch.uint8, device=dev)
    roffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sent = torch.empty(replies.numel(), dtype=torch.uint8, device=dev)
    soffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    scnt = torch.empty(1, dtype=torch.int64, device=dev)
    scof = torch.empty(n, dtype=torch.int32, device=dev)
    sorg = torch.empty(n, dtype=torch.int64, device=dev)
    spos = torch.empty(n, dtype=torch.int64, device=dev)
    squeues = torch.empty(4 * NC, dtype=torch.int64, device=dev)
    scounts = torch.empty(4, dtype=torch.int64, device=dev)
    ws = torch.empty(max(L.xdrg_rpc_recv_batch_workspace_size(NC, size), L.xdrg_rpc_reply_batch_workspace_size(n)),
                     dtype=torch.uint8, device=dev)
    ws2 = torch.empty(L.xdrg_rpc_send_batch_workspace_size(n, NC), dtype=torch.uint8, device=dev)
    st = M.Status(dev)
    outs = (out, offs, cnt, cof, conns, hdrs, replies, roffs, sent, soffs, scnt, scof, sorg, spos, squeues, scounts)

    def four(s):
        R.launch_recv_batch(d_buf, d_segs, RM.MAXLEN, 0, out, offs, cnt, cof, None, conns, st, ws, s)
        A.check(L.xdrg_rpc_dispatch(out.data_ptr(), out.numel(), offs.data_ptr(), n, procs.data_ptr(),
                                    procs.numel() // 4, hdrs.data_ptr(), s), "xdrg_rpc_dispatch")
        R.launch_reply_batch(hdrs, [answers], replies, roffs, None, st, ws, s)
        R.launch_send_batch([R.SendSource(replies, roffs, route)], NC, None, sent, soffs, scnt, scof, sorg, spos,
                            squeues, scounts, st, ws2, s)

    def load(seed):
        buf, segs, to = contents(seed)
        d_buf.zero_()
        d_buf[:buf.size].copy_(torch.from_numpy(buf).to(dev))
        d_segs.copy_(torch.from_numpy(segs.view(np.int64).copy()).to(dev))
        route.copy_(torch.from_numpy(to).to(dev))
        for t in outs:
            t.fill_(0x5A if t.dtype == torch.uint8 else -3)
        ws2.fill_(0x5A)
        torch.cuda.synchronize()
        return to

    def results():
        torch.cuda.synchronize()
        assert int(cnt.item()) == n and int(scnt.item()) == n
        total = int(soffs[n].item())
        return (sent.cpu().numpy()[:total].copy(), soffs.cpu().numpy().copy(), scof.cpu().numpy().copy(),
                sorg.cpu().numpy().copy(), spos.cpu().numpy().copy(), squeues.cpu().numpy().copy(),
                scounts.cpu().numpy().copy(), replies.cpu().numpy()[:int(roffs[n].item())].copy(),
                roffs.cpu().numpy().copy())

    load(0)
    four(torch.cuda.current_stream().cuda_stream)  # outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            four(side.cuda_stream)
    seen, ordered = set(), []
    for seed in (1, 2, 3):
        load(seed)
        four(torch.cuda.current_stream().cuda_stream)
        plain = results()
        to = load(seed)
        graph.replay()
        replayed = results()
        for a, b in zip(plain, replayed):
            assert a.tobytes() == b.tobytes()
        src = {"bytes": replayed[7], "offsets": replayed[8].view(np.uint64), "conn": to.view(np.uint32),
               "count": None, "cap": n}
        want = SM.send_batch([src], NC)
        assert want["count"] == n and replayed[0].tobytes() == want["stream"].tobytes()
        assert np.array_equal(replayed[1].view(np.uint64), want["offsets"])
        assert np.array_equal(replayed[2].view(np.uint32), want["conn_of"])
        assert np.array_equal(replayed[3].view(np.uint64), want["origin"]) and np.array_equal(replayed[4], want["pos"])
        assert replayed[5].tobytes() == want["queues"].tobytes() and tuple(replayed[6].tolist()) == want["counts"]
        ordered.append(bool((np.diff(want["keys"]) >= 0).all()))
        seen.add(replayed[0].tobytes())
        assert st.read(torch.cuda.current_stream().cuda_stream).code == 0
    assert ordered == [True, False, True] and len(seen) == 3  # every replay followed its own bytes and routes
