"""GPU: the asynchronous client over many connections (include/xdrgpu.h "The
asynchronous client over many connections"): xdrg_rpc_socks_next_xids,
_pending_add, _match_replies, _call_stats and _pending_retire.  Every call is
compared bit for bit with the existing single-socket call run on each
socket's part of the same device arrays, and with socks_model (a dict of
per-socket calls_ dicts over the single-socket models); none of the expected
values comes from the code under test.  Integer work: compared exactly."""
import os

import numpy as np
import pytest

from conftest import GOLD

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402
from xdrpp_amd.xdr_types import compile_plan  # noqa: E402
import call_stream_model as CS  # noqa: E402
import oracle_bridge as O  # noqa: E402
import reply_model as RM  # noqa: E402
import settle_model as SM  # noqa: E402
import socks_model as KM  # noqa: E402

SUCCESS = (A.RPCS_ACCEPT_STAT, 0)
GUARD = -2


def g_(name, dtype=np.uint8):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def u64_dev(a, dev):
    return to_dev(np.asarray(a, dtype=np.uint64).view(np.int64), dev)


def i32_dev(a, dev):
    return to_dev((np.asarray(a).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32), dev)


def raw_table(tsock, table, last, dev) -> R.SockCalls:
    """Device arrays as they are (socket numbers at or past nsocks included):
    the caller's order is the table's."""
    return R.SockCalls.from_device(to_dev(table.view(np.int64), dev), i32_dev(tsock, dev),
                                   torch.arange(len(table), dtype=torch.int64, device=dev), i32_dev(last, dev))


def single(p: R.SockCalls, lo: int, hi: int, last_xid: int = 0) -> R.PendingCalls:
    """Entries [lo, hi) of the device table as the single-socket calls take
    them: the same memory, no copy."""
    return R.PendingCalls.from_device(p.table[lo:hi], torch.arange(hi - lo, dtype=torch.int64, device=p.device),
                                      last_xid=last_xid)


def guarded(n: int, dtype, dev):
    """n elements with two guard elements before and after."""
    t = torch.full((n + 4,), GUARD, dtype=dtype, device=dev)
    return t, t[2:n + 2]


def guards_intact(t: torch.Tensor) -> bool:
    h = t.cpu().numpy()
    return bool((h[:2] == GUARD).all() and (h[-2:] == GUARD).all())


# ------------------------------- xdrg_rpc_socks_next_xids and _pending_add
@pytest.mark.parametrize("case", KM.XID_CASES, ids=[c[0] for c in KM.XID_CASES])
@pytest.mark.parametrize("beyond", [False, True])
def test_next_xids_and_pending_add(dev, case, beyond):
    name, socks, xids, res, last, call_sock = case
    if beyond:  # the last two sockets are no sockets: they index nothing and count from 0
        last = last[:max(last.size - 2, 0)]
    nsocks, n = last.size, call_sock.size
    tsock, table, _ = KM.sorted_table(socks, xids, res)
    nc = len(table)
    p = raw_table(tsock, table, last, dev)
    cs = i32_dev(call_sock, dev)
    want_x, want_last = KM.next_xids(tsock, table, last, call_sock)
    # ---- the xids
    xg, x = guarded(n, torch.int32, dev)
    lg, lout = guarded(nsocks, torch.int32, dev)
    R.launch_socks_next_xids(p, cs, x, lout)
    got = x.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want_x) and np.array_equal(lout.cpu().numpy().view(np.uint32), want_last)
    assert guards_intact(xg) and guards_intact(lg)
    x2 = torch.full((n,), GUARD, dtype=torch.int32, device=dev)
    R.launch_socks_next_xids(p, cs, x2, None)  # without d_last_out
    assert torch.equal(x2, x)
    # ---- the merge
    new = np.zeros(n, dtype=R.CALL_DTYPE)
    new["xid"], new["res"] = want_x, (np.arange(n) * 5 + 1) % 61
    new["res"][::9] = A.RPC_RES_UNSENT  # merged like any other entry
    d_new = to_dev(new.view(np.int64), dev)
    mg, merged = guarded(nc + n, torch.int64, dev)
    sg, msock = guarded(nc + n, torch.int32, dev)
    og, old_pos = guarded(nc, torch.int64, dev)
    ng, new_pos = guarded(n, torch.int64, dev)
    R.launch_socks_pending_add(p, d_new, cs, merged, msock, old_pos, new_pos)
    want_sock, want_m, want_old, want_new = KM.pending_add(tsock, table, call_sock, new)
    assert np.array_equal(merged.cpu().numpy().view(R.CALL_DTYPE), want_m)
    assert np.array_equal(msock.cpu().numpy(), want_sock)
    assert np.array_equal(old_pos.cpu().numpy(), want_old) and np.array_equal(new_pos.cpu().numpy(), want_new)
    assert all(guards_intact(t) for t in (mg, sg, og, ng))
    m2, s2 = torch.empty_like(merged), torch.empty_like(msock)
    R.launch_socks_pending_add(p, d_new, cs, m2, s2, None, None)  # without the positions
    assert torch.equal(m2, merged) and torch.equal(s2, msock)
    # ---- socket by socket: the existing calls on the same device memory
    for g in KM.socks_of(tsock, call_sock):
        lo, hi = KM.run_of(tsock, g)
        a, b = KM.run_of(call_sock, g)
        q = single(p, lo, hi, int(last[g]) if g < nsocks else 0)
        one = torch.empty(b - a, dtype=torch.int32, device=dev)
        R.launch_next_xids(q, one)
        assert torch.equal(one, x[a:b]), (name, g)
        om, oo, on = (torch.empty(k, dtype=torch.int64, device=dev) for k in (hi - lo + b - a, hi - lo, b - a))
        R.launch_pending_add(q, d_new[a:b], om, oo, on)
        assert torch.equal(om, merged[lo + a:hi + b]) and bool((msock[lo + a:hi + b] == g).all()), (name, g)
        assert torch.equal(oo + (lo + a), old_pos[lo:hi]) and torch.equal(on + (lo + a), new_pos[a:b]), (name, g)
    if name == "nsocks1" and not beyond:  # the single-socket call itself
        assert np.array_equal(got, CS.next_xids(table["xid"], int(last[0]), n))
    if name == "pending_0_after_wrap" and not beyond:
        assert got.reshape(3, 5).tolist() == [[0xFFFFFFFE, 1, 3, 4, 5]] * 3


def test_call_batch_not_in_socket_order(dev):
    p = R.SockCalls([], [], [], nsocks=3, device=dev)
    idx = u64_dev(np.arange(4), dev)
    for socks in ([0, 2, 1, 2], [0, 1, 2, 3], [-1, 0, 1, 2]):
        with pytest.raises(ValueError):
            R.socks_call_batch(p, socks, [((1, 1, 1), 0, idx, None, 0)])
    with pytest.raises(ValueError):
        R.socks_call_batch(p, [0, 1, 2], [((1, 1, 1), 0, idx, None, 0)])  # four entries, three calls
    s, o, x, p2, ranges = R.socks_call_batch(p, [0, 0, 2, 2], [((1, 1, 1), 7, idx, None, 0)])
    assert x.cpu().tolist() == [1, 2, 1, 2] and ranges.tolist() == [[0, 88], [88, 88], [88, 176]]
    assert p2.calls.tolist() == [(1, 7), (2, 7), (1, 7), (2, 7)] and p2.socks_numpy().tolist() == [0, 0, 2, 2]
    assert p2.last_numpy().tolist() == [2, 0, 2] and s.numel() == 176


# ------------------------------------------- xdrg_rpc_socks_match_replies
@pytest.mark.parametrize("name", KM.MATCH_CASES)
def test_match_replies(dev, name):
    socks, xids, s, o, rows, row_sock, nrows = KM.match_case(name)
    n = o.size - 1
    msock = KM.msg_socks(rows, row_sock, nrows)
    want_h, want_call, want_reply = KM.match(s, o, msock, socks, xids)
    p = R.SockCalls(socks, xids, np.arange(xids.size) % 5, max(nrows, int(socks.max()) + 1), dev)
    st, od = to_dev(s, dev), u64_dev(o, dev)
    hdrs = R.check_replies(st, od)
    before = R.hdrs_numpy(hdrs).copy()
    cg, call = guarded(n, torch.int64, dev)
    rg, reply_of = guarded(p.ncalls, torch.int64, dev)
    R.launch_socks_match_replies(st, od, i32_dev(rows, dev), None if row_sock is None else i32_dev(row_sock, dev),
                                 nrows, p, hdrs, call, reply_of)
    assert guards_intact(cg) and guards_intact(rg)
    h = R.hdrs_numpy(hdrs)
    assert h.tobytes() == want_h.tobytes()
    assert np.array_equal(p.to_caller(call).cpu().numpy(), want_call)
    assert np.array_equal(reply_of[p.inv].cpu().numpy(), want_reply)
    changed = h["action"] != before["action"]
    assert (h["action"][changed] == A.RPCR_UNKNOWN_XID).all() and not changed[want_call >= 0].any()
    # the wrapper, in the caller's positions
    wh, wcall, wreply = R.socks_match_replies(st, od, i32_dev(rows, dev), p,
                                              None if row_sock is None else row_sock.tolist())
    assert np.array_equal(wcall.cpu().numpy(), want_call) and np.array_equal(wreply.cpu().numpy(), want_reply)
    # socket by socket: the existing call on each socket's own messages and its own part of the table
    tsock = p.socks_numpy()
    for g in KM.socks_of(msock):
        mine = np.nonzero(msock == g)[0]
        lo, hi = KM.run_of(tsock, g) if g >= 0 else (0, 0)
        pieces = [s[int(o[i]):int(o[i + 1])] for i in mine]
        sub = np.concatenate(pieces)
        so = np.concatenate([[0], np.cumsum([q.size for q in pieces])]).astype(np.uint64)
        ds, dso = to_dev(sub, dev), u64_dev(so, dev)
        oh = R.check_replies(ds, dso)
        oc = torch.empty(mine.size, dtype=torch.int64, device=dev)
        orp = torch.empty(max(hi - lo, 1), dtype=torch.int64, device=dev)
        R.launch_match_replies(ds, dso, single(p, lo, hi), oh, oc, orp)
        assert np.array_equal(R.hdrs_numpy(oh)["action"], h["action"][mine]), g
        oc, tc = oc.cpu().numpy(), call.cpu().numpy()[mine]
        assert np.array_equal(np.where(oc >= 0, oc + lo, -1), tc), g
        orp, tr = orp[:hi - lo].cpu().numpy(), reply_of.cpu().numpy()[lo:hi]
        assert np.array_equal(np.where(orp >= 0, mine[np.clip(orp, 0, None)], -1), tr), g


def test_match_replies_empty_sides(dev):
    s, o = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    p = R.SockCalls([0, 1], [1, 1], 0, 2, dev)
    reply_of = torch.full((2,), GUARD, dtype=torch.int64, device=dev)
    R.launch_socks_match_replies(to_dev(s, dev), u64_dev(o, dev), torch.empty(0, dtype=torch.int32, device=dev), None,
                                 2, p, torch.empty(0, dtype=torch.uint8, device=dev),
                                 torch.empty(0, dtype=torch.int64, device=dev), reply_of)
    assert reply_of.cpu().tolist() == [-1, -1]  # n == 0: the fill alone
    socks, xids, s, o, rows, _, nrows = KM.match_case("xid1_on_three")
    e = R.SockCalls([], [], [], nrows, dev)
    h, call, _ = R.socks_match_replies(to_dev(s, dev), u64_dev(o, dev), i32_dev(rows, dev), e)
    assert (R.hdrs_numpy(h)["action"] == A.RPCR_UNKNOWN_XID).all() and (call.cpu().numpy() == -1).all()


# ----------------------- xdrg_rpc_socks_call_stats and _pending_retire
def some_headers(n: int) -> np.ndarray:
    h = np.zeros(n, dtype=R.HDR_DTYPE)
    k = np.arange(n)
    h["action"] = np.array([A.RPCR_OK, A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH,
                            A.RPCR_GARBAGE_RES, A.RPCR_UNKNOWN_XID, A.RPCR_MALFORMED])[k % 7]
    h["w"][:, A.RPC_W_STAT], h["w"][:, A.RPC_W_WHY] = 1 + k % 5, 1 + k % 11
    return h


@pytest.mark.parametrize("nc", KM.SIZES)
def test_call_stats_and_retire(dev, nc):
    """Every closed mask crossed with every answered mask; guard words round
    every output; the workspace is dirty.  The existing calls give the same:
    call_stats with either `unanswered` chosen per entry, pending_retire with
    the entries of closed sockets marked answered, and (tables up to 1025)
    both on every socket's part alone."""
    tsock, table, nsocks = KM.settle_table(nc)
    h = some_headers(1000)  # answered values are message numbers below 1000, or no message number at all
    hd = to_dev(h.view(np.uint8), dev)
    p = raw_table(tsock, table, np.zeros(nsocks), dev)
    whole = single(p, 0, nc)
    need = A.lib().xdrg_rpc_socks_pending_retire_workspace_size(nc)
    ws = torch.full((max(need, 16),), 0xA5, dtype=torch.uint8, device=dev)
    for aname in KM.ANSWERED:
        rt = KM.answered(aname, nc)
        d_rt = u64_dev(rt, dev)
        both = []
        for un in (A.RPCS_PENDING, A.RPCS_NETWORK_ERROR):
            t = torch.empty(max(nc, 1), dtype=torch.int64, device=dev)[:nc]
            R.launch_call_stats(hd, d_rt, t, un)
            both.append(t)
        for cname in KM.CLOSED_MASKS:
            closed = KM.closed_mask(cname, nsocks)
            d_closed = i32_dev(closed, dev)
            dead = KM.closed_of(closed, tsock)
            # ---- stats
            sg, stats = guarded(nc, torch.int64, dev)
            R.launch_socks_call_stats(hd, d_rt, p, d_closed, stats)
            assert guards_intact(sg)
            assert np.array_equal(R.call_stats_numpy(stats), KM.call_stats_arrays(h, rt, tsock, closed)), (aname, cname)
            assert torch.equal(stats, torch.where(to_dev(dead, dev), both[1], both[0])), (aname, cname)
            # ---- retire
            kg, kept = guarded(nc, torch.int64, dev)
            ksg, kept_sock = guarded(nc, torch.int32, dev)
            pg, kept_pos = guarded(nc, torch.int64, dev)
            cg, count = guarded(1, torch.int64, dev)
            ws.fill_(0xA5)
            R.launch_socks_pending_retire(p, d_rt, d_closed, kept, kept_sock, kept_pos, count, ws[:need])
            want_kept, want_sock, want_pos, want_count = KM.retire_arrays(tsock, table, rt, closed)
            k = int(count.item())
            assert k == want_count and all(guards_intact(t) for t in (kg, ksg, pg, cg)), (aname, cname)
            assert np.array_equal(kept[:k].cpu().numpy().view(R.CALL_DTYPE), want_kept), (aname, cname)
            assert np.array_equal(kept_sock[:k].cpu().numpy(), want_sock), (aname, cname)
            assert np.array_equal(kept_pos.cpu().numpy().view(np.uint64), want_pos), (aname, cname)
            if nc:
                ok, op, ocount = (torch.empty(m, dtype=torch.int64, device=dev) for m in (nc, nc, 1))
                R.launch_pending_retire(whole, torch.where(to_dev(dead, dev), torch.zeros_like(d_rt), d_rt), ok, op,
                                        ocount, ws)
                assert int(ocount.item()) == k and torch.equal(ok[:k], kept[:k]) and torch.equal(op, kept_pos)
            if 0 < nc <= 1025 and aname == "random":
                at = 0
                for g in KM.socks_of(tsock):
                    lo, hi = KM.run_of(tsock, g)
                    q = single(p, lo, hi)
                    one = torch.empty(hi - lo, dtype=torch.int64, device=dev)
                    R.launch_call_stats(hd, d_rt[lo:hi], one, A.RPCS_NETWORK_ERROR if closed[g] else A.RPCS_PENDING)
                    assert torch.equal(one, stats[lo:hi]), (cname, g)
                    if closed[g]:  # abort_all_calls: calls_.clear()
                        assert bool((kept_pos[lo:hi] == -1).all())
                        continue
                    ok, op, ocount = (torch.empty(m, dtype=torch.int64, device=dev) for m in (hi - lo, hi - lo, 1))
                    R.launch_pending_retire(q, d_rt[lo:hi], ok, op, ocount, ws)
                    c = int(ocount.item())
                    assert torch.equal(ok[:c], kept[at:at + c]) and bool((kept_sock[at:at + c] == g).all()), (cname, g)
                    assert torch.equal(torch.where(op >= 0, op + at, op), kept_pos[lo:hi]), (cname, g)
                    at += c
                assert at == k
    if nc:  # without d_kept_pos; a socket number at or past nsocks counts as open
        few = i32_dev(np.ones(2), dev)  # sockets 0 and 1 closed, every other is no socket
        kept, kept_sock = torch.empty(nc, dtype=torch.int64, device=dev), torch.empty(nc, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        rt = KM.answered("random", nc)
        R.launch_socks_pending_retire(p, u64_dev(rt, dev), few, kept, kept_sock, None, count, ws)
        want_kept, want_sock, _, want_count = KM.retire_arrays(tsock, table, rt, np.ones(2))
        assert int(count.item()) == want_count
        assert np.array_equal(kept[:want_count].cpu().numpy().view(R.CALL_DTYPE), want_kept)
        assert np.array_equal(kept_sock[:want_count].cpu().numpy(), want_sock)
        stats = torch.empty(nc, dtype=torch.int64, device=dev)
        R.launch_socks_call_stats(hd, u64_dev(rt, dev), p, few, stats)
        assert np.array_equal(R.call_stats_numpy(stats), KM.call_stats_arrays(h, rt, tsock, np.ones(2)))


# ------------------------------------------------------------------ rounds
PROCS = {(100000, 2, 0): "rec128", (100000, 3, 1): "recvar", (100003, 3, 5): "containertest"}
NSOCKS, FAILS = 5, 1
RUNS = (190, 130, 0, 257, 191)                   # calls a socket: 768 in all
LAST0 = (0xFFFFFFB0, 0, 9, 0xFFFFFFFF, 0x7FFFFFFF)  # socket 0's xids wrap; sockets 1 and 2 start near each other


class Rounds:
    """768 calls of three procedures to 5 sockets, sent with socks_call_batch;
    every socket's range of the stream served by dispatch -> decode_args ->
    echo -> reply_batch; the replies back as three reads a socket, cut at
    seeded points."""

    def __init__(self, dev):
        self.dev = dev
        self.per, self.keys, self.n = 256, list(PROCS), 768
        self.plans = {key: M.Plan(S.ALL[name]) for key, name in PROCS.items()}
        self.rplans = {p: self.plans[k] for p, k in enumerate(self.keys)}
        self.cps = {p: compile_plan(S.ALL[PROCS[k]]) for p, k in enumerate(self.keys)}
        self.args = [None] * self.n
        self.sources = self.make_sources(self.per, self.args)
        self.socks = np.repeat(np.arange(NSOCKS), RUNS)
        self.res = (np.arange(self.n) % 3).astype(np.uint32)
        self.pending0 = R.SockCalls([], [], [], NSOCKS, dev, last=LAST0)
        calls, offs, xids, self.pending1, self.ranges = R.socks_call_batch(self.pending0, self.socks, self.sources)
        self.xids = xids.cpu().numpy().view(np.uint32)
        self.call_offs = offs.cpu().numpy()
        # every connection's server: its own range of the call stream and nothing else
        self.reply = [None] * self.n
        self.wire = []
        for g in range(NSOCKS):
            a, b = KM.run_of(self.socks, g)
            lo, hi = (int(v) for v in self.ranges[g])
            assert (lo, hi) == (int(self.call_offs[a]), int(self.call_offs[b]))
            if a == b:
                self.wire.append(np.zeros(0, np.uint8))
                continue
            mine = calls[lo:hi].clone()
            hd = R.dispatch(mine, M.index_messages(mine), W.RPC_PROCS)
            decoded = R.decode_args(mine, hd, self.plans)
            results = []
            for key in self.keys:
                index, native, heap = decoded[key]
                results.append((index, M.Marshaler(self.plans[key], dev).encode(native, index.numel(), heap)))
            replies, roffs = R.reply_batch(hd, results)
            rb, ro = replies.cpu().numpy(), roffs.cpu().numpy()
            for c in range(a, b):
                self.reply[c] = rb[int(ro[c - a]):int(ro[c - a + 1])]
                assert RM.be_word(self.reply[c], 4) == int(self.xids[c])
            # the server answers in an order of its own and drops every seventh call
            order = np.random.default_rng(40 + g).permutation(np.arange(a, b))
            self.wire.append(np.concatenate([self.reply[c] for c in order if c % 7 != 3]))
        self.dropped = np.arange(self.n) % 7 == 3

    def make_sources(self, per, args=None):
        out = []
        for p, key in enumerate(self.keys):
            name = PROCS[key]
            nat, heap = W.GENERATORS[name](per)
            index = 3 * ((37 * np.arange(per)) % per) + p  # record k is the argument of call index[k]
            if args is not None:
                x, xo = O.encode(compile_plan(S.ALL[name]), nat, per, heap)
                for k in range(per):
                    args[int(index[k])] = x[int(xo[k]):int(xo[k + 1])]
            enc = M.Marshaler(self.plans[key], self.dev).encode(to_dev(nat, self.dev), per,
                                                                None if heap is None else to_dev(heap, self.dev))
            out.append((key, p, u64_dev(index, self.dev), enc))
        return out

    def reads(self):
        """reads[r][g]: the bytes socket g's r-th read returns.  The cuts are
        seeded byte positions (inside marks and bodies).  Socket FAILS: its
        second read ends, after the rest of the reply the first read cut and
        two whole replies, with a mark whose fragment bit is clear."""
        rng = np.random.default_rng(77)
        out = [[None] * NSOCKS for _ in range(3)]
        self.limit = {}
        for g, w in enumerate(self.wire):
            c1, c2 = sorted(int(v) for v in rng.integers(1, max(w.size, 2), size=2))
            if g == FAILS:
                c1 = int(rng.integers(w.size // 8, w.size // 2))  # most of its replies never arrive
                ends, at = [], 0
                while at < w.size:
                    at += 4 + (RM.be_word(w, at) & 0x7FFFFFFF)
                    ends.append(at)
                first = next(k for k, e in enumerate(ends) if e >= c1)
                stop = ends[first + 2]
                bad = np.array([0x00000010, 1, 2, 3, 4], dtype=">u4").view(np.uint8)
                out[0][g], out[1][g], out[2][g] = w[:c1], np.concatenate([w[c1:stop], bad]), w[stop:]
                self.limit[g] = stop
                assert 0 < first and first + 3 < len(ends)
            else:
                out[0][g], out[1][g], out[2][g] = w[:c1], w[c1:c2], w[c2:]
        return out


@pytest.fixture(scope="module")
def rounds(dev):
    return Rounds(dev)


def same_pending(p: R.PendingCalls, q: R.PendingCalls):
    assert p.ncalls == q.ncalls and p.last_xid == q.last_xid and np.array_equal(p.calls, q.calls)
    assert torch.equal(p.inv, q.inv) and torch.equal(p.perm, q.perm)


def test_rounds(dev, rounds):
    L, n = rounds, rounds.n
    # ---- the send: every socket's xids are those of its own rpc_sock
    for g in range(NSOCKS):
        a, b = KM.run_of(L.socks, g)
        assert np.array_equal(L.xids[a:b], CS.next_xids([], LAST0[g], b - a))
    assert np.count_nonzero(np.diff(L.xids[:RUNS[0]].astype(np.int64)) < 0) == 1      # socket 0 wrapped
    assert np.intersect1d(L.xids[:RUNS[0]], L.xids[RUNS[0]:RUNS[0] + RUNS[1]]).size > 50  # the same xids on two sockets
    p = L.pending1
    want_sock, want_table, _ = KM.sorted_table(L.socks, L.xids, L.res)
    assert np.array_equal(p.calls, want_table) and np.array_equal(p.socks_numpy(), want_sock)
    assert p.last_numpy().tolist() == [int(L.xids[KM.run_of(L.socks, g)[1] - 1]) if RUNS[g] else LAST0[g] for g in range(NSOCKS)]
    with pytest.raises(ValueError):  # what one xid space for all connections makes of this
        R.PendingCalls(L.xids, L.res, dev)
    # ---- five independent single-socket loops beside it
    solo = [p.for_sock(g) for g in range(NSOCKS)]
    solo_orig = [p.callers_of(g) for g in range(NSOCKS)]  # the original call of every call of solo[g]
    fed = [np.zeros(0, np.uint8) for _ in range(NSOCKS)]
    done = [0] * NSOCKS
    # ---- three reads
    rx = R.Receiver()
    closed = None
    orig = np.arange(n)  # the original call of every call of `p`
    final = np.full(n, -1, dtype=np.int64)  # the stat type every call ended with
    final_stat = np.zeros(n, dtype=A.CALL_STAT_DTYPE)
    reads = L.reads()
    for r in range(3):
        for g in range(NSOCKS):
            if g in rx.closed:
                with pytest.raises(ValueError):
                    rx.feed(g, reads[r][g])
                continue
            if reads[r][g].size:
                rx.feed(g, reads[r][g])
                fed[g] = np.concatenate([fed[g], reads[r][g]])
        buf, segs = rx.batch(pin=False)
        got = R.recv_batch(buf.to(dev), segs)
        conns = got.conns_numpy()
        rx.advance(conns)
        ids = list(rx.ids)
        closed = R.closed_socks(got, ids, NSOCKS, also=closed)
        want_closed = [int(g == FAILS and r >= 1) for g in range(NSOCKS)]
        assert closed.cpu().tolist() == want_closed and closed.dtype == torch.int32
        if r == 1:
            assert int(conns["state"][ids.index(FAILS)]) == A.CONN_FRAGMENT and rx.closed == {FAILS: A.CONN_FRAGMENT}
        # the model on what was delivered
        s, o = got.stream.cpu().numpy(), got.offsets.cpu().numpy().astype(np.uint64)
        msock = KM.msg_socks(got.conn_of.cpu().numpy(), ids, len(ids))
        psocks, pxids, pres = L.socks[orig], L.xids[orig], L.res[orig]
        mh, mcall, mreply = KM.match(s, o, msock, psocks, pxids)
        RM.verify_results(s, mh, mcall, pres, L.cps)
        mstats = KM.call_stats(mh, mreply, psocks, want_closed)
        msock2, mtable2, mold, minv = KM.retire(psocks, pxids, pres, mreply, want_closed)
        # every intact reply carries its own call's argument back
        hd, call, reply_of = R.socks_match_replies(got.stream, got.offsets, got.conn_of, p, ids)
        assert np.array_equal(call.cpu().numpy(), mcall) and np.array_equal(reply_of.cpu().numpy(), mreply)
        hh = R.hdrs_numpy(hd)
        for m in np.nonzero(mcall >= 0)[0]:
            assert s[int(hh["body_off"][m]):int(hh["end"][m])].tobytes() == L.args[int(orig[mcall[m]])].tobytes(), (r, m)
        assert (hh["action"][mcall >= 0] == A.RPCR_OK).all() and np.count_nonzero(mcall >= 0) == got.count
        # ---- settle
        stats, results, p2, old_of_new = R.socks_settle(got, p, L.rplans, closed, ids=ids)
        st = R.call_stats_numpy(stats)
        assert np.array_equal(st, mstats)
        assert np.array_equal(old_of_new.cpu().numpy(), mold)
        assert np.array_equal(p2.calls, mtable2) and np.array_equal(p2.socks_numpy(), msock2)
        assert np.array_equal(p2.inv.cpu().numpy(), minv) and torch.equal(p2.last, p.last)
        assert sum(v[0].numel() for v in results.values()) == got.count
        index, native, _ = results[0]  # rec128: message m carries the record of the call it answers
        sent_rec = {int(3 * ((37 * k) % L.per)): k for k in range(L.per)}
        recs = [sent_rec[int(orig[mcall[m]])] for m in index.cpu().numpy()]
        assert np.array_equal(native.cpu().numpy().reshape(-1, 128), W.rec128(L.per)[0].reshape(-1, 128)[recs])
        settled = st["type"] != A.RPCS_PENDING
        assert (final[orig[settled]] == -1).all()  # nobody's callback runs twice
        final[orig[settled]], final_stat[orig[settled]] = st["type"][settled], st[settled]
        # ---- the same round in every socket's own loop: the messages its bytes hold so far, past those it had
        for g in range(NSOCKS):
            aborted = g == FAILS and r >= 1
            have = fed[g][:L.limit[g]] if g == FAILS else fed[g]
            ends, at = [], 0
            while at + 4 <= have.size and at + 4 + (RM.be_word(have, at) & 0x7FFFFFFF) <= have.size:
                at += 4 + (RM.be_word(have, at) & 0x7FFFFFFF)
                ends.append(at)
            begin = ends[done[g] - 1] if done[g] else 0
            sub = have[begin:at]
            so = (np.array([begin] + ends[done[g]:], dtype=np.int64) - begin).astype(np.uint64)
            done[g] = len(ends)
            if g == FAILS and r == 2:
                sub, so = np.zeros(0, np.uint8), np.zeros(1, np.uint64)  # nothing is read from a closed socket
            gstats, _, q2, gold = R.settle(to_dev(sub, dev), u64_dev(so, dev), solo[g], L.rplans, aborted=aborted)
            mine = np.nonzero(psocks == g)[0]
            assert np.array_equal(orig[mine], solo_orig[g]), (r, g)
            assert np.array_equal(st[mine], R.call_stats_numpy(gstats)), (r, g)
            same_pending(p2.for_sock(g), q2)
            solo[g], solo_orig[g] = q2, solo_orig[g][gold.cpu().numpy()]
        p, orig = p2, orig[mold]
    # ---- what every call came to
    wire_calls = [set() for _ in range(NSOCKS)]
    at = 0
    w = L.wire[FAILS]
    by_xid = {int(L.xids[c]): c for c in np.nonzero(L.socks == FAILS)[0]}
    while at < L.limit[FAILS]:
        wire_calls[FAILS].add(by_xid[RM.be_word(w, at + 4)])
        at += 4 + (RM.be_word(w, at) & 0x7FFFFFFF)
    on_fail = L.socks == FAILS
    counted = np.isin(np.arange(n), list(wire_calls[FAILS]))
    assert (final[on_fail & counted] == A.RPCS_ACCEPT_STAT).all() and (final_stat["stat"][on_fail & counted] == 0).all()
    assert (final[on_fail & ~counted] == A.RPCS_NETWORK_ERROR).all() and np.count_nonzero(on_fail & ~counted) > 20
    assert (final[~on_fail & ~L.dropped] == A.RPCS_ACCEPT_STAT).all() and (final[~on_fail & L.dropped] == -1).all()
    assert not (final == A.RPCS_NETWORK_ERROR)[~on_fail].any()  # no other socket is touched
    left = np.nonzero(~on_fail & L.dropped)[0]
    assert np.array_equal(orig, left) and p.ncalls == left.size and not (p.socks_numpy() == FAILS).any()
    # ---- the next round: every socket counts on from its own xid_ over what it still has pending
    near = p.last_numpy().copy()
    for g in (0, 3):  # a full turn of the counter later the xids meet the table again
        near[g] = (int(L.xids[left[L.socks[left] == g]].min()) - 3) & 0xFFFFFFFF
    p = R.SockCalls.from_device(p.table, p.sock, p.inv, i32_dev(near, dev))
    socks2 = np.repeat(np.arange(NSOCKS), (100, 60, 30, 70, 40))
    _, _, xids2, p3, ranges2 = R.socks_call_batch(p, socks2, L.make_sources(100))
    x2 = xids2.cpu().numpy().view(np.uint32)
    for g in range(NSOCKS):
        a, b = KM.run_of(socks2, g)
        q = p.for_sock(g)
        assert q.last_xid == int(near[g])
        one = torch.empty(b - a, dtype=torch.int32, device=dev)
        R.launch_next_xids(q, one)
        assert np.array_equal(one.cpu().numpy().view(np.uint32), x2[a:b]), g
        assert np.array_equal(x2[a:b], CS.next_xids(L.xids[left[L.socks[left] == g]], int(near[g]), b - a))
    assert np.isin(L.xids[left[L.socks[left] == 0]], (int(near[0]) + 1 + np.arange(100)) & 0xFFFFFFFF).any()  # some are met
    assert not np.isin(x2[:100], L.xids[left[L.socks[left] == 0]]).any()                                      # and skipped
    assert p3.ncalls == left.size + 300 and np.array_equal(ranges2[1:, 0], ranges2[:-1, 1])
    want_sock3, want_table3, _ = KM.sorted_table(np.concatenate([L.socks[left], socks2]),
                                                 np.concatenate([L.xids[left], x2]),
                                                 np.concatenate([L.res[left], np.arange(300) % 3]))
    assert np.array_equal(p3.calls, want_table3) and np.array_equal(p3.socks_numpy(), want_sock3)


# ----------------------------------------------------------------- edges
def settled(dev, socks, xids, res, last, s, o, rows, closed, plans, cps):
    """socks_settle() on a small table against socks_model; returns (stats as
    numpy, results, pending2, old_of_new)."""
    nsocks = len(last)
    p = R.SockCalls(socks, xids, res, nsocks, dev, last=last)
    mh, mcall, mreply = KM.match(s, o, KM.msg_socks(rows, None, nsocks), socks, xids)
    RM.verify_results(s, mh, mcall, np.broadcast_to(np.asarray(res, dtype=np.int64), (len(xids),)), cps)
    mstats = KM.call_stats(mh, mreply, socks, closed)
    msock2, mtable2, mold, minv = KM.retire(socks, xids, res, mreply, closed)
    hd, call, reply_of = R.socks_match_replies(to_dev(s, dev), u64_dev(o, dev), i32_dev(rows, dev), p)
    assert R.hdrs_numpy(hd).tobytes() == mh.tobytes()  # no reply here has a result to verify
    assert np.array_equal(call.cpu().numpy(), mcall) and np.array_equal(reply_of.cpu().numpy(), mreply)
    assert call.dtype == reply_of.dtype == torch.int64
    stats, results, p2, old_of_new = R.socks_settle((to_dev(s, dev), u64_dev(o, dev), i32_dev(rows, dev)), p, plans,
                                                    i32_dev(closed, dev))
    assert stats.dtype == torch.int64 and np.array_equal(R.call_stats_numpy(stats), mstats)
    assert old_of_new.dtype == torch.int64 and np.array_equal(old_of_new.cpu().numpy(), mold)
    assert p2.ncalls == len(mtable2) and np.array_equal(p2.calls, mtable2) and np.array_equal(p2.socks_numpy(), msock2)
    assert np.array_equal(p2.inv.cpu().numpy(), minv) and np.array_equal(p2.perm.cpu().numpy(), np.argsort(minv))
    assert p2.nsocks == nsocks and torch.equal(p2.last, p.last) and p2.last_numpy().tolist() == list(last)
    assert p2.table.dtype == torch.int64 and p2.sock.dtype == torch.int32
    return mh, R.call_stats_numpy(stats), results, p2, old_of_new


@pytest.mark.parametrize("closed", [(0, 0, 0), (0, 1, 0)])
@pytest.mark.parametrize("nmsgs", [0, 2])
def test_settle_on_an_empty_table(dev, nmsgs, closed):
    s, o = KM.reply_stream([5, 0xFFFFFFFE][:nmsgs])
    plans, cps = {0: None, 1: M.Plan(S.rec128)}, {0: None, 1: compile_plan(S.rec128)}
    mh, st, results, p2, old_of_new = settled(dev, [], [], [], [7, 0, 0xFFFFFFF0], s, o, np.array([0, 2][:nmsgs]),
                                              np.array(closed), plans, cps)
    assert len(mh) == nmsgs and (mh["action"] == A.RPCR_UNKNOWN_XID).all()
    assert len(st) == 0 and p2.ncalls == 0 and old_of_new.numel() == 0
    assert sorted(results) == [0, 1] and all(v[0].numel() == 0 and v[0].dtype == torch.int64 for v in results.values())
    assert results[0][1:] == (None, None)
    assert results[1][1].numel() == 0 and results[1][1].dtype == torch.uint8 and results[1][2] is None


def test_settle_that_leaves_no_call(dev):
    """3 calls over 2 sockets, each answered or on the closed socket: count is
    0, and the stats come in the caller's order."""
    socks, xids = np.array([1, 0, 1]), np.array([5, 5, 9])
    s, o = KM.reply_stream([9, 5])
    _, st, results, p2, old_of_new = settled(dev, socks, xids, 0, [5, 9], s, o, np.array([1, 0]), np.array([0, 1]),
                                             {0: None}, {0: None})
    assert st.tolist() == [(A.RPCS_NETWORK_ERROR, 0), SUCCESS, SUCCESS]
    assert p2.ncalls == 0 and old_of_new.numel() == 0
    assert results[0][0].cpu().tolist() == [0, 1] and results[0][1:] == (None, None)


def test_call_batch_of_no_calls(dev):
    """n = 0 and no sources on a table of 2 calls: an empty stream, and the
    table as it was."""
    p = R.SockCalls([2, 0], [7, 7], [1, 0], 3, dev, last=[7, 0, 0xFFFFFFFE])
    stream, offs, xids, p2, ranges = R.socks_call_batch(p, [], [])
    assert stream.numel() == 0 and stream.dtype == torch.uint8 and offs.cpu().tolist() == [0]
    assert xids.numel() == 0 and xids.dtype == torch.int32
    assert ranges.tolist() == [[0, 0]] * 3 and ranges.dtype == np.int64
    assert p2.ncalls == 2 and p2.nsocks == 3 and np.array_equal(p2.calls, p.calls)
    for a in ("table", "sock", "inv", "perm", "last"):
        assert torch.equal(getattr(p2, a), getattr(p, a)), a
    assert p2.calls.tolist() == [(7, 0), (7, 1)] and p2.socks_numpy().tolist() == [0, 2]


# ---------------------------------------------------------- graph capture
def test_graph_capture(dev):
    """One capture of launch_socks_match_replies -> launch_verify_results ->
    launch_socks_call_stats -> launch_socks_pending_retire on a single stream,
    replayed over other reply bytes and another `closed`."""
    n, nsocks = 512, 4
    msgs = g_(f"success_rec128_{n}.msgs").copy()
    offsets = np.arange(n + 1, dtype=np.uint64) * 156
    xid = (np.arange(n, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    rows = np.arange(n) % nsocks
    spare = np.setdiff1d(np.arange(0x100, 0x400, dtype=np.uint32), xid)[:100]
    # message k < 200 is pending on the socket it arrives on, messages 200..259 on the next one only
    socks = np.concatenate([rows[:200], (rows[200:260] + 1) % nsocks, np.arange(100) % nsocks])
    xids = np.concatenate([xid[:260], spare])
    p = R.SockCalls(socks, xids, 0, nsocks, dev)
    nc = p.ncalls
    plan, cp = M.Plan(S.rec128), compile_plan(S.rec128)
    st, od, d_rows = to_dev(msgs, dev), u64_dev(offsets, dev), i32_dev(rows, dev)
    d_closed = torch.zeros(nsocks, dtype=torch.int32, device=dev)
    hdrs = torch.empty(n * A.RPC_HDR_BYTES, dtype=torch.uint8, device=dev)
    call = torch.empty(n, dtype=torch.int64, device=dev)
    reply_of, stats, kept, kept_pos = (torch.empty(nc, dtype=torch.int64, device=dev) for _ in range(4))
    kept_sock = torch.empty(nc, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(A.lib().xdrg_rpc_socks_pending_retire_workspace_size(nc), 16), dtype=torch.uint8, device=dev)

    def four(stream=None):
        R.launch_socks_match_replies(st, od, d_rows, None, nsocks, p, hdrs, call, reply_of, stream)
        R.launch_verify_results(st, hdrs, call, p, [plan], 0, A.DEFAULT_STACK_LIMIT, None, stream)
        R.launch_socks_call_stats(hdrs, reply_of, p, d_closed, stats, stream)
        R.launch_socks_pending_retire(p, reply_of, d_closed, kept, kept_sock, kept_pos, count, ws, stream)

    hdrs.copy_(R.check_replies(st, od))
    four()  # the plan's first launch, outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            four(side.cuda_stream)
    counts = []
    for rnd in range(2):
        closed = np.zeros(nsocks, dtype=np.int64)
        if rnd == 1:  # other bytes: 50 spare calls get a reply on socket k % 4; and sockets 1 and 3 have failed
            be = msgs.reshape(n, 156)
            be[300:350, 4:8] = spare[:50].astype(">u4").view(np.uint8).reshape(50, 4)
            st.copy_(to_dev(msgs, dev))
            closed[[1, 3]] = 1
            d_closed.copy_(i32_dev(closed, dev))
        hdrs.copy_(R.check_replies(st, od))
        for t in (stats, kept, kept_pos, count, reply_of, call):
            t.fill_(-3)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want_h, want_call, want_reply = KM.match(msgs, offsets, rows, socks, xids)
        RM.verify_results(msgs, want_h, want_call, np.zeros(nc, np.int64), {0: cp})
        want_stats = KM.call_stats(want_h, want_reply, socks, closed)
        want_sock, want_table, want_old, want_inv = KM.retire(socks, xids, 0, want_reply, closed)
        assert R.hdrs_numpy(hdrs).tobytes() == want_h.tobytes()
        assert np.array_equal(reply_of[p.inv].cpu().numpy(), want_reply)
        assert np.array_equal(R.call_stats_numpy(stats[p.inv]), want_stats)
        k = int(count.item())
        assert k == len(want_table) and np.array_equal(kept[:k].cpu().numpy().view(R.CALL_DTYPE), want_table)
        assert np.array_equal(kept_sock[:k].cpu().numpy(), want_sock)
        want_pos = np.full(nc, -1, dtype=np.int64)
        want_pos[want_old] = want_inv
        assert np.array_equal(kept_pos[p.inv].cpu().numpy(), want_pos)
        ty = want_stats["type"]
        counts.append((k, int(np.count_nonzero(ty == A.RPCS_PENDING)), int(np.count_nonzero(ty == A.RPCS_NETWORK_ERROR)),
                       int(np.count_nonzero(want_stats == np.array(SUCCESS, dtype=want_stats.dtype)))))
    # 200 answered and 160 waiting (60 replies arrived on the wrong socket); then the 50 new replies find their
    # calls (spare call j sits on socket j % 4, where message 300 + j arrives), and the 110 still unanswered split
    # into the open sockets', which stay, and the failed sockets'
    assert counts[0] == (160, 160, 0, 200)
    assert counts[1][3] == 250 and counts[1][1] + counts[1][2] == 110 and counts[1][0] == counts[1][1] and counts[1][2] > 40
