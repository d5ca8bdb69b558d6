"""GPU: xdrg_rpc_recv_batch against the host model (tests/recv_model.py, held
to the reference by test_recv_model.py), bit for bit: stream, offsets, count,
conn_of, kind and every field of every xdrg_rpc_conn record."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD

from xdrpp_amd import _abi as A
from xdrpp_amd import marshal as M
from xdrpp_amd import rpc as R
import msg_streams as MS
import recv_model as RM

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64  # canary elements either side of an output


def guarded(n: int, dtype, dev):
    """(whole, view): n elements with PAD canary elements either side."""
    fill = CANARY if dtype == torch.uint8 else 0x25A5A5A5
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    return whole, whole[PAD:PAD + n]


def intact(whole: torch.Tensor, n: int) -> bool:
    w = whole.cpu().numpy()
    fill = CANARY if whole.dtype == torch.uint8 else 0x25A5A5A5
    return bool((w[:PAD] == fill).all() and (w[PAD + n:] == fill).all())


def run(dev, buf: np.ndarray, segs, maxlen=RM.MAXLEN, rpc=False, cap=None, max_msgs=None, with_kind=None):
    """One call through the launch_ mirror with canaries round d_out,
    d_offsets, d_conn_of and d_kind.  segs: a numpy table (sent as it is: no
    host check).  Returns a dict of numpy results and the status."""
    segs = np.ascontiguousarray(segs).view(A.CONN_IN_DTYPE).reshape(-1)
    nconns = segs.size
    cap = buf.size if cap is None else cap
    max_msgs = buf.size // 4 if max_msgs is None else max_msgs
    with_kind = rpc if with_kind is None else with_kind
    d_buf = torch.from_numpy(np.ascontiguousarray(buf)).to(dev)
    d_segs = torch.from_numpy(segs.view(np.int64).copy()).to(dev)
    out_w, out = guarded(cap, torch.uint8, dev)
    offs_w, offs = guarded(max_msgs + 1, torch.int64, dev)
    cof_w, cof = guarded(max_msgs, torch.int32, dev)
    kind_w, kind = guarded(max_msgs, torch.uint8, dev)
    cnt = torch.full((1,), -7, dtype=torch.int64, device=dev)
    conns = torch.full((max(4 * nconns, 4),), -7, dtype=torch.int64, device=dev)[:4 * nconns]
    ws = torch.empty(max(A.lib().xdrg_rpc_recv_batch_workspace_size(nconns, buf.size), 16), dtype=torch.uint8,
                     device=dev)
    st = M.Status(dev)
    s = torch.cuda.current_stream().cuda_stream
    st.init(s)
    R.launch_recv_batch(d_buf, d_segs, maxlen, A.RECV_RPC_SOCK if rpc else 0, out, offs, cnt, cof,
                        kind if with_kind else None, conns, st, ws, s)
    e = st.read(s)
    n = int(cnt.item())
    assert intact(out_w, cap) and intact(offs_w, max_msgs + 1) and intact(cof_w, max_msgs) and intact(kind_w, max_msgs)
    assert 0 <= n <= max_msgs
    return {"stream": out.cpu().numpy(), "offsets": offs.cpu().numpy().view(np.uint64), "count": n,
            "conn_of": cof.cpu().numpy().view(np.uint32), "kind": kind.cpu().numpy() if with_kind else None,
            "conns": R.conns_numpy(conns), "code": int(e.code), "record": int(e.record),
            "total_bytes": int(e.total_bytes)}


def same(got, want, rpc):
    """got (run()) equals the model's (stream, offsets, conn_of, kind, conns) bit for bit."""
    stream, offsets, conn_of, kind, conns = want
    assert got["code"] == 0, (got["code"], got["record"])
    n = offsets.size - 1
    assert got["count"] == n and got["total_bytes"] == stream.size
    assert np.array_equal(got["offsets"][:n + 1], offsets)
    assert np.array_equal(got["conn_of"][:n], conn_of)
    if rpc:
        assert np.array_equal(got["kind"][:n], kind)
    assert got["conns"].tobytes() == conns.tobytes(), \
        [(i, a, b) for i, (a, b) in enumerate(zip(got["conns"].tolist(), conns.tolist())) if a != b][:5]
    assert got["stream"][:stream.size].tobytes() == stream.tobytes()


def check(dev, conn_bytes, maxlen=RM.MAXLEN, rpc=False, align=16):
    buf, segs = RM.pack(conn_bytes, align)
    got = run(dev, buf, segs, maxlen, rpc)
    want = RM.recv_batch(buf, segs, maxlen, rpc)
    same(got, want, rpc)
    return got, want


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLD, "recv.json")) as f:
        d = json.load(f)
    return d["max_msg_len"], [RM.connection(c["seed"], c["sizes"], c["edits"].get("frag"), c["edits"].get("cut", 0))
                              for c in d["connections"]]


# ---------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("rpc", [False, True])
@pytest.mark.parametrize("nconns", [None, 1, 63, 64, 65, 257])
def test_fixture_batches(dev, fixture, nconns, rpc):
    """The reference-pinned connections as one batch, and repeated to 1, 63,
    64, 65 and 257 connections: the wave and tile edges."""
    maxlen, xs = fixture
    conns = xs if nconns is None else [xs[(i + 2) % len(xs)] for i in range(nconns)]
    got, want = check(dev, conns, maxlen, rpc, align=4 if nconns == 63 else 16)
    if nconns is None:
        states = set(want[4]["state"].tolist())
        assert states == ({RM.OPEN, RM.FRAGMENT, RM.TOO_LONG, RM.BAD_RPC} if rpc else
                          {RM.OPEN, RM.FRAGMENT, RM.TOO_LONG})


# ----------------------------------------------------------- 2. isolation
def good_conns(n=80):
    return [RM.connection(100 + i, [8, 40, 8][:1 + i % 3] + [12] * (i % 2), cut=(5 if i % 7 == 3 else 0))
            for i in range(n)]


def failing(kind: int) -> np.ndarray:
    rng = np.random.default_rng(50 + kind)
    g = [RM.message(rng, s, word1=k) for s, k in ((8, 0), (40, 1), (16, 0), (8, 1))]
    bad = {RM.FRAGMENT: RM.message(rng, 24, frag=True, word1=0), RM.TOO_LONG: RM.message(rng, 5000, word1=0)[:40],
           RM.BAD_SIZE: RM.message(rng, 22, word1=0), RM.BAD_RPC: RM.message(rng, 24, word1=2)}[kind]
    return np.concatenate(g[:2] + [bad] + g[2:])


@pytest.fixture(scope="module")
def good_alone(dev):
    return check(dev, good_conns(), 4096, True)


@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("kind", [RM.FRAGMENT, RM.TOO_LONG, RM.BAD_SIZE, RM.BAD_RPC])
def test_one_bad_connection_closes_itself_only(dev, good_alone, kind, lane):
    good = good_conns()
    base_got, _ = good_alone
    got, _ = check(dev, good[:lane] + [failing(kind)] + good[lane:], 4096, True)
    rec = got["conns"][lane]
    assert (int(rec["state"]), int(rec["msgs"]), int(rec["consumed"]), int(rec["need"])) == (kind, 2, 12 + 44, 0)
    f = int(rec["first"])
    assert got["stream"][int(got["offsets"][f]):int(got["offsets"][f + 2])].tobytes() == failing(kind)[:56].tobytes()
    assert (got["conn_of"][:got["count"]] == lane).sum() == 2          # the two before the failure, none after
    others = np.delete(got["conns"], lane)
    for field in ("consumed", "msgs", "need", "state"):
        assert np.array_equal(others[field], base_got["conns"][field]), field
    keep = got["conn_of"][:got["count"]] != lane

    def messages(r, mask=None):
        o = r["offsets"]
        ks = range(r["count"]) if mask is None else np.nonzero(mask)[0]
        return [r["stream"][int(o[k]):int(o[k + 1])].tobytes() for k in ks]
    assert messages(got, keep) == messages(base_got)
    assert np.array_equal(got["kind"][:got["count"]][keep], base_got["kind"][:base_got["count"]])


# ------------------------------------------- 3. one connection = the index
STATE_OF_ERR = {A.ERR_MSG_EOF: RM.OPEN, A.ERR_MSG_FRAGMENT: RM.FRAGMENT, A.ERR_MSG_TOO_LONG: RM.TOO_LONG}


@pytest.mark.parametrize("name,maxlen", [("mixed", MS.MIB), ("mixed", 20 * MS.KIB), ("mixed", 16380),
                                         ("trunc_long", MS.MIB), ("frag", MS.MIB), ("alternating", MS.MIB)])
def test_one_connection_equals_the_index(dev, name, maxlen):
    """Messages of 16,380, 16,384, 20 KiB and 1 MiB, at and past an LDS
    window, with body words that read as marks."""
    x = MS.stream(name)
    segs = np.array([(0, x.size)], dtype=A.CONN_IN_DTYPE)
    got = run(dev, x, segs, maxlen, False)
    same(got, RM.recv_batch(x, segs, maxlen, False), False)
    rec = got["conns"][0]
    try:
        offs = M.index_messages(torch.from_numpy(x).to(dev), maxlen).cpu().numpy().view(np.uint64)
        assert np.array_equal(got["offsets"][:got["count"] + 1], offs)
        assert (int(rec["state"]), int(rec["need"]), int(rec["consumed"])) == (RM.OPEN, 0, x.size)
    except M.XdrBadMessageSize as e:  # the index stops at the same message
        assert e.record == got["count"] and STATE_OF_ERR[e.code] == int(rec["state"])
        assert int(rec["consumed"]) < x.size
    with open(os.path.join(GOLD, "frames.json")) as f:
        fr = [r for r in json.load(f)["framings"] if r["stream"] == name and r["max_msg_len"] == maxlen][0]
    assert got["offsets"][:got["count"] + 1].tolist() == fr["offsets"]
    assert got["stream"][:int(rec["consumed"])].tobytes() == x[:int(rec["consumed"])].tobytes()
    if name == "trunc_long":
        assert (int(rec["state"]), int(rec["need"])) == (RM.OPEN, 4 + MS.MIB)


# ------------------------------------------- 4. lane pass to wave pass
@pytest.mark.parametrize("rpc", [False, True])
def test_lane_pass_to_wave_pass(dev, rpc):
    """kRbLaneBytes = 1024 (recv_batch_kernels.h): a connection of at most
    that many bytes is walked by its lane, a longer one by a wave through
    windows of kRbWinBytes = 16384.  8-byte messages take 12 bytes: 85 of them
    are 1020 bytes."""
    assert RM.LANE_BYTES == 1024 and RM.WIN_BYTES == 16384
    per = RM.LANE_BYTES // 12
    small = [RM.connection(300 + i, [8] * (1 + i % 4), cut=(i % 3) * 5) for i in range(24)]
    edge = [RM.connection(400, [8] * (per - 1)), RM.connection(401, [8] * per),
            RM.connection(402, [8] * (per + 1), cut=8),            # 1024 bytes: the last lane-pass length
            RM.connection(403, [8] * (per + 1), cut=7),            # 1025
            RM.connection(404, [8] * (per + 1)), RM.connection(405, [8] * (per + 2), cut=10)]
    assert [e.size for e in edge] == [1008, 1020, 1024, 1025, 1032, 1034]
    wins = [RM.connection(406, [8] * (RM.WIN_BYTES // 12)),         # 16380: one window
            RM.connection(407, [8] * (RM.WIN_BYTES // 12 + 1)),     # a mark in the window's last word
            RM.connection(408, [RM.WIN_BYTES - 4]), RM.connection(409, [RM.WIN_BYTES, 8]),
            RM.connection(410, [8, RM.WIN_BYTES - 16, 8, 8])]
    long_ = [RM.connection(411, [8] * 5000), RM.connection(412, [8, 20 * MS.KIB] * 300)]
    conns = small[:8] + edge + small[8:12] + wins + small[12:16] + long_ + small[16:]
    assert len(conns) <= 64  # one wave: small connections before and after the long ones
    check(dev, conns, MS.MIB, rpc)


# ------------------------------------------------------- 5. the scan's carry
def one_message_batch(n: int):
    """n connections of one 8-byte message at a 12-byte stride, connection 7
    cut inside its mark, the last one without the fragment bit; and what the
    call gives, built with array operations."""
    m = np.zeros((n, 12), dtype=np.uint8)
    m[:, 0], m[:, 3] = 0x80, 8
    m[:, 4:8] = (np.arange(n, dtype=np.uint32) * 2654435761).astype(">u4").view(np.uint8).reshape(n, 4)
    m[:, 11] = np.arange(n) % 2
    m[n - 1, 0] = 0
    segs = np.zeros(n, dtype=A.CONN_IN_DTYPE)
    segs["begin"] = np.arange(n, dtype=np.uint64) * 12
    segs["len"] = 12
    segs["len"][7] = 2
    whole = np.ones(n, dtype=bool)
    whole[[7, n - 1]] = False
    conns = np.zeros(n, dtype=A.CONN_DTYPE)
    conns["msgs"] = whole
    conns["consumed"] = 12 * whole
    conns["first"] = np.cumsum(whole) - whole
    conns["need"][7] = 4
    conns["state"][n - 1] = RM.FRAGMENT
    k = int(whole.sum())
    want = (m[whole].reshape(-1), np.arange(k + 1, dtype=np.uint64) * 12, np.nonzero(whole)[0].astype(np.uint32),
            (np.nonzero(whole)[0] % 2).astype(np.uint8), conns)
    return m.reshape(-1), segs, want


def test_scan_carry(dev):
    """256 * 1024 + 1 connections: the smallest batch that needs the second
    round of k_tile_scan."""
    buf, segs, want = one_message_batch(300)
    model = RM.recv_batch(buf, segs, RM.MAXLEN, True)
    for a, b in zip(want, model):  # the array form is the model's
        assert a.tobytes() == b.tobytes()
    n = RM.TILE * RM.SCAN_LANES + 1
    buf, segs, want = one_message_batch(n)
    got = run(dev, buf, segs, RM.MAXLEN, True)
    same(got, want, True)
    assert got["count"] == n - 2 and int(got["conns"]["first"][-1]) == n - 2


# ------------------------------------------------- 6. rounds, end to end
def g(name, dtype=np.uint8):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


def rebased(hdrs: np.ndarray, marks) -> np.ndarray:
    """Headers with body_off and end counted from each message's mark (a
    malformed header's body_off is 0 and stays)."""
    h = hdrs.copy()
    marks = np.asarray(marks, dtype=np.uint64)
    h["body_off"] -= np.where(h["body_off"] != 0, marks, np.uint64(0))
    h["end"] -= marks
    return h


NC, ROUNDS = 37, 5


def dealt_calls():
    """rpccall_1024.stream's messages dealt to NC connections, and each
    connection's ROUNDS - 1 seeded cut points."""
    stream = g("rpccall_1024.stream")
    msgs, consumed, _, state = RM.frame(stream)
    assert len(msgs) == 1024 and consumed == stream.size and state == RM.OPEN
    whole = [stream[p:p + b] for p, b, _ in msgs]
    dealt = [list(range(c, 1024, NC)) for c in range(NC)]
    data = [np.concatenate([whole[i] for i in d]) for d in dealt]
    rng = np.random.default_rng(37)
    cuts = [np.sort(rng.integers(0, x.size + 1, ROUNDS - 1)).tolist() for x in data]
    first = [whole[d[0]].size for d in dealt]
    cuts[0][0] = first[0]                                   # exactly at a mark
    cuts[1][0] = first[1] + 2                               # inside a mark
    cuts[2][:2] = [first[2] + 9, first[2] + 10]             # inside a body, then one byte more: held back by need
    return whole, dealt, data, [sorted(c) for c in cuts]


def feed_rounds(data, cuts, recv):
    """Feed every connection through Receiver in ROUNDS rounds; recv(buf,
    segs) -> (stream, offsets, conns, extra).  Returns per connection its
    (message bytes, extra(k)) in delivery order and what the cuts were."""
    rx = R.Receiver()
    seen = {"mark": 0, "body": 0, "at_mark": 0, "held": 0}
    out = [[] for _ in data]
    for r in range(ROUNDS):
        for c, x in enumerate(data):
            lo = cuts[c][r - 1] if r else 0
            hi = cuts[c][r] if r < ROUNDS - 1 else x.size
            rx.feed(c, x[lo:hi].tobytes())
        buf, segs = rx.batch(pin=False)
        ids = rx.ids
        seen["held"] += sum(1 for c in range(len(data)) if rx.pending(c) and c not in ids)
        st, offs, conns, extra = recv(buf, segs)
        for i, c in enumerate(ids):
            f, k = int(conns["first"][i]), int(conns["msgs"][i])
            out[c] += [(st[int(offs[j]):int(offs[j + 1])].tobytes(), extra(j)) for j in range(f, f + k)]
            if r < ROUNDS - 1:
                need, left = int(conns["need"][i]), int(segs["len"][i]) - int(conns["consumed"][i])
                seen["mark"] += need == 4
                seen["body"] += need > 4
                seen["at_mark"] += need == 0 and left == 0
        assert (conns["state"] == RM.OPEN).all()
        rx.advance(conns)
    assert all(rx.pending(c) == 0 for c in range(len(data))) and not rx.closed
    return out, seen


def model_recv(buf, segs):
    st, offs, _, _, conns = RM.recv_batch(buf.numpy(), segs, RM.MAXLEN, False)
    return st, offs, conns, lambda j: None


def test_rounds_on_the_reference_calls(dev):
    """rpccall_1024.stream dealt to 37 connections and fed through Receiver
    in 5 rounds: every message is delivered once, in order within its
    connection, and dispatch's headers are the reference's (body_off and end
    counted from the message's mark, since a message's place in the stream is
    the batch's).  Without recv_msg's test: the reference's calls include
    malformed ones, which dispatch is there to drop and which would close
    their connections here."""
    ref_hdrs = g("rpccall_1024.hdrs").view(R.HDR_DTYPE)
    procs = g("rpc_procs.bin", "<u4").reshape(-1, 4)
    whole, dealt, data, cuts = dealt_calls()
    out, seen = feed_rounds(data, cuts, model_recv)  # the seeds' conditions, on the model, before the GPU sees anything
    assert all(v > 0 for v in seen.values()), seen
    assert [[m for m, _ in o] for o in out] == [[whole[i].tobytes() for i in d] for d in dealt]

    def gpu(buf, segs):
        got = R.recv_batch(buf.to(dev), segs, rpc_sock=False)
        want = RM.recv_batch(buf.numpy(), segs, RM.MAXLEN, False)
        st, offs = got.stream.cpu().numpy(), got.offsets.cpu().numpy().view(np.uint64)
        assert st.tobytes() == want[0].tobytes() and np.array_equal(offs, want[1])
        assert np.array_equal(got.conn_of.cpu().numpy().view(np.uint32), want[2])
        assert got.kind is None and got.conns_numpy().tobytes() == want[4].tobytes()
        if got.count == 0:
            return st, offs, got.conns_numpy(), lambda j: None
        hd = R.dispatch(got.stream, got.offsets, procs)
        rows = rebased(R.hdrs_numpy(hd), offs[:-1])
        replies, ro = R.reply_batch(hd, [])
        rr = got.reply_ranges(ro)
        assert rr[0, 0] == 0 and rr[-1, 1] == replies.numel() and (rr[1:, 0] == rr[:-1, 1]).all()  # tiles the stream
        ron, cn = ro.cpu().numpy(), got.conns_numpy()
        first, cnt = cn["first"].astype(np.int64), cn["msgs"].astype(np.int64)
        assert np.array_equal(rr[:, 1] - rr[:, 0], ron[first + cnt] - ron[first])
        return st, offs, cn, lambda j: rows[j].tobytes()
    out, seen2 = feed_rounds(data, cuts, gpu)
    assert seen2 == seen
    marks = np.cumsum([0] + [w.size for w in whole[:-1]]).astype(np.uint64)
    ref = rebased(ref_hdrs, marks)
    assert any(len(set(ref["action"][d].tolist())) > 1 for d in dealt)  # not one kind of header only
    for c, d in enumerate(dealt):
        assert [m for m, _ in out[c]] == [whole[i].tobytes() for i in d]
        assert [h for _, h in out[c]] == [ref[i].tobytes() for i in d], c


# ------------------------------------------------------------ 7. capacity
def test_capacity(dev, fixture):
    maxlen, xs = fixture
    buf, segs = RM.pack([xs[(i + 2) % len(xs)] for i in range(65)])
    stream, offsets, conn_of, kind, conns = RM.recv_batch(buf, segs, maxlen, True)
    n = offsets.size - 1
    assert n > 64
    # 4 bytes short: the last message does not fit, the ones before it are there
    got = run(dev, buf, segs, maxlen, True, cap=stream.size - 4)
    assert (got["code"], got["record"]) == (A.ERR_OVERFLOW_PUT, n - 1)
    assert got["conns"].tobytes() == conns.tobytes() and got["count"] == n
    assert np.array_equal(got["offsets"][:n + 1], offsets) and np.array_equal(got["conn_of"][:n], conn_of)
    last = int(offsets[n - 1])
    assert got["stream"][:last].tobytes() == stream[:last].tobytes()
    assert (got["stream"][last:] == CANARY).all()                  # nothing of the message that does not fit
    assert got["total_bytes"] == stream.size                       # what the stream needs
    # one entry short
    got = run(dev, buf, segs, maxlen, True, max_msgs=n - 1)
    assert (got["code"], got["record"]) == (A.ERR_MSG_COUNT, n - 1)
    assert got["conns"].tobytes() == conns.tobytes() and got["count"] == n - 1
    assert np.array_equal(got["offsets"][:n], offsets[:n]) and np.array_equal(got["conn_of"][:n - 1], conn_of[:n - 1])
    assert np.array_equal(got["kind"][:n - 1], kind[:n - 1])
    # exactly enough of both is no error
    got = run(dev, buf, segs, maxlen, True, cap=stream.size, max_msgs=n)
    same(got, (stream, offsets, conn_of, kind, conns), True)


# ----------------------------------------------------- 8. a table that lies
def clamped(segs: np.ndarray, buf_len: int) -> np.ndarray:
    """rb_seg (recv_batch_kernels.h): begin into the buffer and down to a
    multiple of 4, len to what is left."""
    t = segs.copy()
    top = buf_len & ~3
    t["begin"] = np.minimum(t["begin"], np.uint64(top)) & ~np.uint64(3)
    t["len"] = np.minimum(t["len"], np.uint64(buf_len) - t["begin"])
    return t


@pytest.mark.parametrize("lie", ["len_past_the_buffer", "out_of_order", "begin_past_the_buffer", "misaligned",
                                 "overlapping"])
def test_a_table_that_lies(dev, fixture, lie):
    """The device table is not what the host was promised.  No read leaves
    d_buf: every segment goes through rb_seg's clamp before its first byte is
    read, and the copy reads only bytes the walk consumed.  What can be tested
    is that the call returns what the clamped table gives and that the
    canaries round every output hold (run() asserts them)."""
    maxlen, xs = fixture
    buf, segs = RM.pack([xs[(i + 2) % len(xs)] for i in range(70)] + [RM.connection(9, [8] * 200)])
    buf = buf[:buf.size - 3]  # a length that is no multiple of 4
    n = segs.size
    R.check_segs(np.concatenate([segs[:-1], np.array([(segs["begin"][-1], buf.size - int(segs["begin"][-1]))],
                                                     dtype=A.CONN_IN_DTYPE)]), buf.size)  # a host-valid shape
    if lie == "len_past_the_buffer":
        segs["len"][n - 1] = 1 << 62
        segs["len"][n - 2] = buf.size
    elif lie == "out_of_order":
        segs[[3, 40]] = segs[[40, 3]]
        segs[[n - 1, 0]] = segs[[0, n - 1]]
    elif lie == "begin_past_the_buffer":
        segs["begin"][5], segs["begin"][n - 1] = buf.size + 4096, (1 << 64) - 4
    elif lie == "misaligned":
        segs["begin"][4:9] += np.array([1, 2, 3, 1, 2], dtype=np.uint64)
    else:
        segs["len"][2:30] += 40
    t = clamped(segs, buf.size)
    want = RM.recv_batch(buf, t, maxlen, True)
    got = run(dev, buf, segs, maxlen, True, cap=3 * buf.size, max_msgs=buf.size)
    same(got, want, True)


# ------------------------------------------------------- 9. graph capture
def test_graph_capture(dev):
    """One capture of launch_recv_batch -> xdrg_rpc_dispatch, replayed over
    changed buffer contents and a changed table (without recv_msg's test, as
    in test_rounds_on_the_reference_calls; d_kind is NULL)."""
    stream = g("rpccall_1024.stream")
    procs_np = g("rpc_procs.bin", "<u4").reshape(-1, 4)
    msgs, _, _, _ = RM.frame(stream)
    n = 1024

    def contents(seed):
        """The 1,024 calls dealt to NC connections in a seeded order; some
        connections end in a cut message, one in a cleared fragment bit."""
        rng = np.random.default_rng(seed)
        order = rng.permutation(n)
        parts = [[stream[msgs[i][0]:msgs[i][0] + msgs[i][1]] for i in order[c::NC]] for c in range(NC)]
        for c in range(0, NC, 5):
            parts[c].append(RM.message(rng, 40, word1=0)[:int(rng.integers(1, 40))])
        parts[5 * int(rng.integers(0, 7)) + 1].append(RM.message(rng, 16, frag=True))  # not a cut one
        return RM.pack([np.concatenate(p) for p in parts])

    size = max(contents(s)[0].size for s in range(4))
    d_buf = torch.zeros(size, dtype=torch.uint8, device=dev)
    d_segs = torch.zeros(2 * NC, dtype=torch.int64, device=dev)
    max_msgs = size // 4
    out = torch.empty(size, dtype=torch.uint8, device=dev)
    offs = torch.empty(max_msgs + 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    cof = torch.empty(max_msgs, dtype=torch.int32, device=dev)
    conns = torch.empty(4 * NC, dtype=torch.int64, device=dev)
    hdrs = torch.empty(n * A.RPC_HDR_BYTES, dtype=torch.uint8, device=dev)
    procs = torch.from_numpy(np.ascontiguousarray(procs_np, dtype=np.uint32).view(np.int32)).to(dev)
    ws = torch.empty(A.lib().xdrg_rpc_recv_batch_workspace_size(NC, size), dtype=torch.uint8, device=dev)
    st = M.Status(dev)

    def two(s):
        R.launch_recv_batch(d_buf, d_segs, RM.MAXLEN, 0, out, offs, cnt, cof, None, conns, st, ws, s)
        A.check(A.lib().xdrg_rpc_dispatch(out.data_ptr(), out.numel(), offs.data_ptr(), n, procs.data_ptr(),
                                          procs.numel() // 4, hdrs.data_ptr(), s), "xdrg_rpc_dispatch")

    def load(seed):
        buf, segs = contents(seed)
        d_buf.zero_()
        d_buf[:buf.size].copy_(torch.from_numpy(buf).to(dev))
        d_segs.copy_(torch.from_numpy(segs.view(np.int64).copy()).to(dev))
        for t in (out, offs, cnt, cof, conns, hdrs):
            t.fill_(0x5A if t.dtype == torch.uint8 else -3)
        torch.cuda.synchronize()
        return np.concatenate([buf, np.zeros(size - buf.size, np.uint8)]), segs

    def results():
        torch.cuda.synchronize()
        k = int(cnt.item())
        return (k, out.cpu().numpy(), offs.cpu().numpy()[:k + 1].copy(), cof.cpu().numpy()[:k].copy(),
                conns.cpu().numpy().copy(), hdrs.cpu().numpy().copy())

    load(0)
    two(torch.cuda.current_stream().cuda_stream)  # outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            two(side.cuda_stream)
    seen = set()
    for seed in (1, 2, 3):
        buf, segs = load(seed)
        two(torch.cuda.current_stream().cuda_stream)
        plain = results()
        load(seed)
        graph.replay()
        replayed = results()
        assert plain[0] == replayed[0] == n
        total = int(plain[2][-1])
        assert plain[1][:total].tobytes() == replayed[1][:total].tobytes()
        for a, b in zip(plain[2:], replayed[2:]):
            assert a.tobytes() == b.tobytes()
        want = RM.recv_batch(buf, segs, RM.MAXLEN, False)
        assert replayed[1][:total].tobytes() == want[0].tobytes() and np.array_equal(replayed[2].view(np.uint64), want[1])
        assert replayed[4].tobytes() == want[4].tobytes()
        assert (want[4]["state"] == RM.FRAGMENT).sum() == 1 and (want[4]["need"] > 0).sum() >= 7
        seen.add(replayed[5].tobytes())
        assert st.read(torch.cuda.current_stream().cuda_stream).code == 0
    assert len(seen) == 3  # every replay followed its own bytes
