"""GPU: settling a reply batch (xdrg_rpc_call_stats, xdrg_rpc_pending_retire;
include/xdrgpu.h "Settling a reply batch"): every pending call's
rpc_call_stat in one device array, and calls_ after recv_msg's erases
(xdrpp/msgsock.cc:217-219), so that a client that stays up for a second batch
treats a late duplicate as a reply to an unknown call and hands out the xids
rpc_sock would.

Expected values: settle_model (a dict walked in message order, and the array
form of the three passes), reply_model, call_stream_model and the
reference-written fixtures (rpc_1024.msgs, success_rec128_512.msgs); none
from the code under test.  Integer work: compared exactly."""
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


def g(name, dtype=np.uint8):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def u64_dev(a, dev):
    return to_dev(np.asarray(a, dtype=np.uint64).view(np.int64), dev)


def same_pending(p: R.PendingCalls, q: R.PendingCalls):
    assert p.ncalls == q.ncalls and p.device == q.device and p.last_xid == q.last_xid
    assert np.array_equal(p.calls, q.calls)
    for a in ("table", "perm", "inv"):
        assert torch.equal(getattr(p, a), getattr(q, a)), a


# ------------------------------------------------ xdrg_rpc_pending_retire
@pytest.mark.parametrize("nc", SM.SIZES)
def test_retire_sizes_and_masks(dev, nc):
    """d_kept[:count], d_kept_pos and *d_count against the model for every
    answer mask; one entry before d_kept and everything from d_kept + ncalls
    on stay untouched; the workspace is dirty."""
    xids, res = SM.case_table(nc)
    table, _ = SM.sorted_table(xids, res)
    p = R.PendingCalls(xids, res, dev)
    assert np.array_equal(p.calls, table)
    need = A.lib().xdrg_rpc_pending_retire_workspace_size(nc)
    for name in SM.MASKS:
        rt = SM.answered_values(SM.answered_mask(name, nc))
        want_kept, want_pos, want_count, _ = SM.retire_arrays(table, rt)
        kept = torch.full((nc + 3,), -2, dtype=torch.int64, device=dev)
        pos = torch.full((nc + 2,), -2, dtype=torch.int64, device=dev)
        count = torch.full((3,), -2, dtype=torch.int64, device=dev)
        ws = torch.full((max(need, 16),), 0xA5, dtype=torch.uint8, device=dev)
        R.launch_pending_retire(p, u64_dev(rt, dev), kept[1:nc + 1], pos[1:nc + 1], count[1:2], ws[:need])
        assert count.cpu().tolist() == [-2, want_count, -2], name
        k = kept.cpu().numpy()
        assert k[0] == -2 and (k[nc + 1:] == -2).all(), name
        assert np.array_equal(k[1:1 + want_count].view(R.CALL_DTYPE), want_kept), name
        q = pos.cpu().numpy()
        assert q[0] == q[-1] == -2 and np.array_equal(q[1:-1].view(np.uint64), want_pos), name
    if nc:  # without d_kept_pos
        kept = torch.full((nc,), -2, dtype=torch.int64, device=dev)
        R.launch_pending_retire(p, u64_dev(rt, dev), kept, None, count[1:2], ws)
        assert count[1].item() == want_count
        assert np.array_equal(kept[:want_count].cpu().numpy().view(R.CALL_DTYPE), want_kept)


@pytest.mark.parametrize("case", ["empty", "all_answered", "random"])
def test_retire_against_the_host_constructor(dev, case):
    rng = np.random.default_rng(3)
    nc = {"empty": 0, "all_answered": 300, "random": 1000}[case]
    xids, res = SM.case_table(nc)
    p = R.PendingCalls(xids, res, dev, last_xid=0xFFFFFFF7)
    reply_of = {"empty": np.zeros(0, np.int64), "all_answered": rng.permutation(nc).astype(np.int64),
                "random": np.where(rng.random(nc) < 0.5, rng.integers(0, 5000, size=nc), -1)}[case]
    q, old_of_new = p.retire(to_dev(reply_of, dev))
    want_table, want_old, want_inv = SM.retire(xids, res, reply_of)
    assert np.array_equal(old_of_new.cpu().numpy(), want_old) and old_of_new.dtype == torch.int64
    assert np.array_equal(q.calls, want_table) and np.array_equal(q.inv.cpu().numpy(), want_inv)
    same_pending(q, R.PendingCalls(xids[want_old], res[want_old], dev, last_xid=0xFFFFFFF7))
    assert p.ncalls == nc and np.array_equal(p.calls, SM.sorted_table(xids, res)[0])  # the old table is left alone


# ---------------------------------------------------- xdrg_rpc_call_stats
def golden_replies(extra: int):
    """rpc_1024.msgs and the pending table of test_all_reply_kinds (every
    second reply's xid), with `extra` calls no message answers."""
    m, mo = g("rpc_1024.msgs"), g("rpc_1024.msgoffs", "<u8")
    n = mo.size - 1
    words = np.array([[RM.be_word(m, int(mo[i]) + 4), RM.be_word(m, int(mo[i]) + 8)] if mo[i + 1] - mo[i] >= 12
                      else [0, 0xFFFFFFFF] for i in range(n)], dtype=np.uint64)
    replies = np.nonzero(words[:, 1] == 1)[0]
    assert replies.size == 481
    xids = words[replies[::2], 0].astype(np.uint32)
    free = np.setdiff1d(np.arange(0x7000, 0x7000 + 2000, dtype=np.uint32), words[:, 0].astype(np.uint32))[:extra]
    xids = np.concatenate([xids, free])
    return m, mo, xids[np.random.default_rng(9).permutation(xids.size)]


@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("result", ["void", "rec128"])
def test_call_stats_on_the_reference_bytes(dev, result, extra):
    m, mo, xids = golden_replies(extra)
    cp = None if result == "void" else compile_plan(S.rec128)
    plan = None if result == "void" else M.Plan(S.rec128)
    st, od = to_dev(m, dev), u64_dev(mo, dev)
    pending = R.PendingCalls(xids, 0, dev)
    hd, call, reply_of = R.match_replies(st, od, pending)
    R.verify_results(st, hd, call, pending, {0: plan})
    want_h, want_call, want_reply, want, _ = SM.settle(m, mo, xids, 0, {0: cp})
    assert R.hdrs_numpy(hd).tobytes() == want_h.tobytes() and np.array_equal(reply_of.cpu().numpy(), want_reply)
    assert np.count_nonzero(want_reply < 0) == extra
    before = hd.clone()
    got = R.call_stats_numpy(R.call_stats(hd, reply_of, pending))
    assert np.array_equal(got, want)
    kinds = set(zip(want["type"].tolist(), (want["stat"] != 0).tolist()))
    assert {(A.RPCS_ACCEPT_STAT, True), (A.RPCS_AUTH_STAT, True), (A.RPCS_RPCVERS_MISMATCH, False)} <= kinds
    assert (SUCCESS[0], False) in kinds if result == "void" else (A.RPCS_GARBAGE_RES, False) in kinds
    assert ((A.RPCS_PENDING, False) in kinds) == (extra > 0)
    aborted = R.call_stats_numpy(R.call_stats(hd, reply_of, pending, aborted=True))
    assert np.array_equal(aborted, SM.settle(m, mo, xids, 0, {0: cp}, aborted=True)[3])
    assert np.array_equal(aborted[want_reply >= 0], want[want_reply >= 0])
    assert (aborted["type"][want_reply < 0] == A.RPCS_NETWORK_ERROR).all()
    assert torch.equal(hd, before)  # the headers are read only


@pytest.mark.parametrize("ncalls", [1, 64, 65, 257])
def test_call_stats_of_what_is_no_message_of_the_batch(dev, ncalls):
    """reply_of at or past n is GARBAGE_RES and reads no header: d_hdrs holds
    exactly n records.  Raw launch, table order."""
    n = 5
    h = np.zeros(n, dtype=R.HDR_DTYPE)
    h["action"] = [A.RPCR_OK, A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH, A.RPCR_UNKNOWN_XID]
    h["w"][:, A.RPC_W_STAT], h["w"][:, A.RPC_W_WHY] = [0, 4, 1, 0, 0], [7, 7, 13, 7, 7]
    hd = to_dev(h.view(np.uint8), dev)
    assert hd.numel() == n * A.RPC_HDR_BYTES
    far = np.array([n, n + 1, 1 << 32, 1 << 40, 1 << 63, 0xFFFFFFFFFFFFFFFE, A.RPC_NO_CALL], dtype=np.uint64)
    j = np.arange(ncalls, dtype=np.uint64)
    rt = np.where(j % 3 == 0, far[(j // 3) % far.size], j % n)  # uint64 throughout
    for unanswered, aborted in ((A.RPCS_PENDING, False), (A.RPCS_NETWORK_ERROR, True)):
        stats = torch.full((ncalls + 2,), -2, dtype=torch.int64, device=dev)
        R.launch_call_stats(hd, u64_dev(rt, dev), stats[1:-1], unanswered)
        got = stats.cpu().numpy()
        assert got[0] == got[-1] == -2
        assert np.array_equal(got[1:-1].view(A.CALL_STAT_DTYPE), SM.call_stats(h, rt, aborted))
    if ncalls >= 64:
        want = SM.call_stats(h, rt)
        assert {(0, 0), (0, 4), (A.RPCS_AUTH_STAT, 13), (A.RPCS_RPCVERS_MISMATCH, 0), (A.RPCS_GARBAGE_RES, 0),
                (A.RPCS_PENDING, 0)} == set(want.tolist())


def test_call_stats_without_messages(dev):
    """n == 0 with d_hdrs NULL: every call is unanswered, or GARBAGE_RES
    where reply_of names a message there is not."""
    rt = np.full(65, A.RPC_NO_CALL, dtype=np.uint64)
    rt[[0, 64]] = 0, 3
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    for unanswered, aborted in ((A.RPCS_PENDING, False), (A.RPCS_NETWORK_ERROR, True)):
        stats = torch.full((65,), -2, dtype=torch.int64, device=dev)
        R.launch_call_stats(empty, u64_dev(rt, dev), stats, unanswered)
        assert np.array_equal(R.call_stats_numpy(stats), SM.call_stats(np.zeros(0, R.HDR_DTYPE), rt, aborted))
    p = R.PendingCalls(np.arange(65, dtype=np.uint32) * 3, 0, dev)
    got = R.call_stats_numpy(R.call_stats(empty, torch.full((65,), -1, dtype=torch.int64, device=dev), p, aborted=True))
    assert got.tolist() == [(A.RPCS_NETWORK_ERROR, 0)] * 65


# -------------------------------------------------------------- two rounds
PROCS = {(100000, 2, 0): "rec128", (100000, 3, 1): "recvar", (100003, 3, 5): "containertest"}
LAST = 0xFFFFFF00  # the 768 xids wrap


class Loop:
    """768 calls of three procedures sent with call_batch, as the whole-loop
    test of test_gpu_call_batch.py builds them, and the server's reply to
    every one of them, call by call, on the host."""

    def __init__(self, dev):
        self.dev = dev
        self.per, self.keys = 256, list(PROCS)
        self.n = 3 * self.per
        self.plans = {key: M.Plan(S.ALL[name]) for key, name in PROCS.items()}
        self.rplans = {p: self.plans[k] for p, k in enumerate(self.keys)}
        self.cps = {p: compile_plan(S.ALL[PROCS[k]]) for p, k in enumerate(self.keys)}
        self.args = [None] * self.n
        self.sources = self.make_sources(self.per, self.args)
        self.pending0 = R.PendingCalls(np.zeros(0, np.uint32), np.zeros(0, np.uint32), dev, last_xid=LAST)
        calls, offs, xids, self.pending1 = R.call_batch(self.pending0, self.sources, self.n)
        self.xids = xids.cpu().numpy().view(np.uint32)
        self.res = (np.arange(self.n) % 3).astype(np.uint32)
        # the server answers every call; reply c is the message of call c
        hd = R.dispatch(calls, M.index_messages(calls), W.RPC_PROCS)
        decoded = R.decode_args(calls, hd, self.plans)
        results = []
        for key in self.keys:
            index, native, heap = decoded[key]
            results.append((index, M.Marshaler(self.plans[key], dev).encode(native, index.numel(), heap)))
        replies, roffs = R.reply_batch(hd, results)
        rb, ro = replies.cpu().numpy(), roffs.cpu().numpy()
        self.reply = [rb[int(ro[c]):int(ro[c + 1])] for c in range(self.n)]
        assert all(RM.be_word(r, 4) == int(self.xids[c]) for c, r in enumerate(self.reply))

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

    def stream(self, calls):
        """The replies to `calls`, in that order, as the socket delivers them."""
        s = np.concatenate([self.reply[int(c)] for c in calls] + [np.zeros(0, np.uint8)])
        o = np.concatenate([[0], np.cumsum([self.reply[int(c)].size for c in calls])]).astype(np.uint64)
        return s, o

    def settle(self, s, o, pending, **kw):
        return R.settle(to_dev(s, self.dev), u64_dev(o, self.dev), pending, self.rplans, **kw)


@pytest.fixture(scope="module")
def loop(dev):
    return Loop(dev)


@pytest.fixture(scope="module")
def round1(loop):
    """Two calls of every three answered, in shuffled order, and settled."""
    c = np.arange(loop.n)
    answered = (c // 3 + c % 3) % 3 != 0  # the unanswered one goes round the three procedures
    order = np.random.default_rng(21).permutation(np.nonzero(answered)[0])
    s, o = loop.stream(order)
    return answered, order, s, o, loop.settle(s, o, loop.pending1)


def test_two_rounds(dev, loop, round1):
    n, p1 = loop.n, loop.pending1
    assert np.array_equal(loop.xids, CS.next_xids([], LAST, n)) and np.count_nonzero(np.diff(loop.xids.astype(np.int64)) < 0) == 1
    assert p1.last_xid == int(loop.xids[-1])
    # ---- round 1
    answered, order, s1, o1, (stats, results, p2, old_of_new) = round1
    assert np.count_nonzero(answered) == 512 and all(np.count_nonzero(answered & (loop.res == k)) > 150 for k in range(3))
    _, _, want_reply, want_stats, (want_table, want_old, want_inv) = SM.settle(s1, o1, loop.xids, loop.res, loop.cps)
    got = R.call_stats_numpy(stats)
    assert np.array_equal(got, want_stats)
    assert (got[answered] == np.array(SUCCESS, dtype=got.dtype)).all() and (got["type"][~answered] == A.RPCS_PENDING).all()
    assert np.array_equal(old_of_new.cpu().numpy(), np.nonzero(~answered)[0]) and np.array_equal(want_old, np.nonzero(~answered)[0])
    assert p2.ncalls == 256 and p2.last_xid == p1.last_xid
    assert np.array_equal(p2.calls, want_table) and np.array_equal(p2.inv.cpu().numpy(), want_inv)
    same_pending(p2, R.PendingCalls(loop.xids[want_old], loop.res[want_old], dev, last_xid=p1.last_xid))
    index, native, _ = results[0]  # rec128: message m carries the record of the call it answers
    sent_rec = {int(3 * ((37 * k) % loop.per)): k for k in range(loop.per)}
    recs = [sent_rec[int(order[m])] for m in index.cpu().numpy()]
    assert np.array_equal(native.cpu().numpy().reshape(-1, 128), W.rec128(loop.per)[0].reshape(-1, 128)[recs])
    # ---- round 2, part one: 100 late duplicates among the replies to the other 256
    rng = np.random.default_rng(22)
    dup = rng.permutation(np.nonzero(answered)[0])[:100]
    rest = np.nonzero(~answered)[0]
    msgs = rng.permutation(np.concatenate([dup, rest]))  # message m answers old call msgs[m]
    is_dup = np.isin(msgs, dup)
    s2, o2 = loop.stream(msgs)
    d2, od2 = to_dev(s2, dev), u64_dev(o2, dev)
    hd, call, reply_of, out = R.decode_results(d2, od2, p2, loop.rplans)
    h = R.hdrs_numpy(hd)
    call = call.cpu().numpy()
    assert (h["action"][is_dup] == A.RPCR_UNKNOWN_XID).all() and (call[is_dup] == -1).all()
    new_of_old = np.full(n, -1)
    new_of_old[want_old] = np.arange(256)
    assert (h["action"][~is_dup] == A.RPCR_OK).all() and np.array_equal(call[~is_dup], new_of_old[msgs[~is_dup]])
    assert np.array_equal(np.sort(reply_of.cpu().numpy()), np.nonzero(~is_dup)[0])
    for m in np.nonzero(~is_dup)[0]:  # every one of the 256 carries its own argument back
        assert s2[int(h["body_off"][m]):int(h["end"][m])].tobytes() == loop.args[int(msgs[m])].tobytes(), m
    assert sum(v[0].numel() for v in out.values()) == 256
    mh, mcall, _ = RM.match(s2, o2, loop.xids[want_old])
    assert np.array_equal(mcall, call) and np.array_equal(mh["action"], h["action"])
    # what this change removes for callers: against the unretired table the duplicates do match
    uh, ucall, _ = R.match_replies(d2, od2, p1)
    assert np.array_equal(ucall.cpu().numpy(), msgs) and not (R.hdrs_numpy(uh)["action"] == A.RPCR_UNKNOWN_XID).any()
    # ---- round 2, part two: the table is empty, the xids count on from last_xid
    stats2, _, p3, old3 = R.settle(d2, od2, p2, loop.rplans)
    assert R.call_stats_numpy(stats2).tolist() == [SUCCESS] * 256
    assert p3.ncalls == 0 and old3.numel() == 0 and p3.last_xid == p1.last_xid
    more = loop.make_sources(100)
    _, _, xids3, p4 = R.call_batch(p3, more, 300)
    want3 = CS.next_xids([], p1.last_xid, 300)
    assert np.array_equal(xids3.cpu().numpy().view(np.uint32), want3)
    same_pending(p4, R.PendingCalls(want3, np.arange(300) % 3, dev, last_xid=int(want3[-1])))
    # ---- the variant: 50 calls stay unanswered
    quiet = rest[rng.permutation(256)[:50]]
    sv, ov = loop.stream(msgs[~np.isin(msgs, quiet)])
    statsv, _, pv, oldv = loop.settle(sv, ov, p2)
    assert np.array_equal(want_old[oldv.cpu().numpy()], np.sort(quiet)) and pv.ncalls == 50
    gv = R.call_stats_numpy(statsv)
    assert np.count_nonzero(gv["type"] == A.RPCS_PENDING) == 50 and np.count_nonzero(gv == np.array(SUCCESS, dtype=gv.dtype)) == 206
    assert np.array_equal(gv, SM.settle(sv, ov, loop.xids[want_old], loop.res[want_old], loop.cps)[3])
    _, _, xidsv, _ = R.call_batch(pv, more, 300)
    assert np.array_equal(xidsv.cpu().numpy().view(np.uint32), CS.next_xids(loop.xids[quiet], p1.last_xid, 300))
    # a full turn of the counter later the xids meet the table again: exactly those 50 are skipped
    pv.last_xid = LAST - 20
    _, _, xidsw, _ = R.call_batch(pv, more, 300)
    wantw = CS.next_xids(loop.xids[quiet], LAST - 20, 300)
    assert np.array_equal(xidsw.cpu().numpy().view(np.uint32), wantw)
    assert np.array_equal(wantw, SM.next_xids(loop.xids[want_old], np.where(np.isin(want_old, quiet), -1, 0), LAST - 20, 300))
    assert np.isin(wantw, loop.xids[answered]).any() and not np.isin(wantw, loop.xids[quiet]).any()
    assert not np.array_equal(wantw, CS.next_xids(loop.xids, LAST - 20, 300))  # the table that only grows hands out others


def test_abort(dev, loop, round1):
    """abort_all_calls after round 1: an empty reply stream, aborted."""
    answered, _, _, _, (_, _, p2, old_of_new) = round1
    none, zero = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    stats, results, p3, old3 = loop.settle(none, zero, p2, aborted=True)
    assert R.call_stats_numpy(stats).tolist() == [(A.RPCS_NETWORK_ERROR, 0)] * 256
    assert p3.ncalls == 0 and old3.numel() == 0 and p3.last_xid == p2.last_xid == loop.pending1.last_xid
    assert all(v[0].numel() == 0 for v in results.values())
    # with replies in the batch: the answered calls keep their stats, the rest are NETWORK_ERROR
    some = old_of_new.cpu().numpy()[::4]
    s, o = loop.stream(some)
    stats, _, p3, old3 = loop.settle(s, o, p2, aborted=True)
    got = R.call_stats_numpy(stats)
    want = SM.settle(s, o, loop.xids[~answered], loop.res[~answered], loop.cps, aborted=True)
    assert np.array_equal(got, want[3]) and len(want[4][0]) == 0
    assert got[::4].tolist() == [SUCCESS] * 64 and (np.delete(got, np.s_[::4])["type"] == A.RPCS_NETWORK_ERROR).all()
    assert p3.ncalls == 0 and old3.numel() == 0 and p3.last_xid == p2.last_xid
    plain = R.call_stats_numpy(loop.settle(s, o, p2)[0])
    assert np.array_equal(plain[::4], got[::4]) and (np.delete(plain, np.s_[::4])["type"] == A.RPCS_PENDING).all()


# ----------------------------------------------------------------- edges
@pytest.mark.parametrize("aborted", [False, True])
@pytest.mark.parametrize("nmsgs", [0, 2])
def test_settle_on_an_empty_table(dev, nmsgs, aborted):
    """settle(), decode_results() and retire() with no pending call: every
    well-formed reply is a reply to an unknown call, and everything per call
    comes back empty with last_xid kept."""
    s, o = KM.reply_stream([5, 0xFFFFFFFE][:nmsgs])
    none = np.zeros(0, np.uint32)
    plans, cps = {0: None, 1: M.Plan(S.rec128)}, {0: None, 1: compile_plan(S.rec128)}
    want_h, want_call, want_reply, want_stats, (want_table, want_old, want_inv) = SM.settle(s, o, none, none, cps,
                                                                                          aborted=aborted)
    assert len(want_h) == nmsgs and (want_h["action"] == A.RPCR_UNKNOWN_XID).all() and (want_call == -1).all()
    assert len(want_reply) == len(want_stats) == len(want_table) == len(want_old) == len(want_inv) == 0
    p = R.PendingCalls(none, none, dev, last_xid=0xFFFFFFF7)
    empty = R.PendingCalls(none, none, dev, last_xid=0xFFFFFFF7)
    st, od = to_dev(s, dev), u64_dev(o, dev)
    stats, results, p2, old_of_new = R.settle(st, od, p, plans, aborted=aborted)
    assert stats.numel() == 0 and stats.dtype == torch.int64 and len(R.call_stats_numpy(stats)) == 0
    same_pending(p2, empty)
    assert old_of_new.numel() == 0 and old_of_new.dtype == torch.int64
    assert sorted(results) == [0, 1] and all(v[0].numel() == 0 and v[0].dtype == torch.int64 for v in results.values())
    assert results[0][1:] == (None, None)
    assert results[1][1].numel() == 0 and results[1][1].dtype == torch.uint8 and results[1][2] is None
    hd, call, reply_of, out = R.decode_results(st, od, p, plans)
    assert R.hdrs_numpy(hd).tobytes() == want_h.tobytes() and np.array_equal(call.cpu().numpy(), want_call)
    assert call.dtype == torch.int64 and reply_of.numel() == 0 and reply_of.dtype == torch.int64
    assert all(v[0].numel() == 0 for v in out.values())
    assert R.call_stats(hd, reply_of, p, aborted).numel() == 0
    q, old = p.retire(reply_of)
    same_pending(q, empty)
    assert old.numel() == 0 and old.dtype == torch.int64


def test_call_batch_of_no_calls(dev):
    """n = 0 and no sources on a table of 2 calls: an empty stream, and the
    table as it was."""
    p = R.PendingCalls([0xFFFFFFFE, 7], [1, 0], dev, last_xid=0xFFFFFFFE)
    assert CS.next_xids(p.calls["xid"], p.last_xid, 0).size == 0
    stream, offs, xids, p2 = R.call_batch(p, [])
    assert stream.numel() == 0 and stream.dtype == torch.uint8 and offs.cpu().tolist() == [0]
    assert xids.numel() == 0 and xids.dtype == torch.int32
    same_pending(p2, p)
    assert p2.calls.tolist() == [(7, 0), (0xFFFFFFFE, 1)] and p2.inv.cpu().tolist() == [1, 0]
    same_pending(R.call_batch(p, [], 0)[3], p)


# ---------------------------------------------------------- graph capture
def test_graph_capture(dev):
    """One capture of launch_match_replies -> launch_verify_results ->
    launch_call_stats -> launch_pending_retire on a single stream, replayed
    over reply bytes in which a different set of calls is answered."""
    n = 512
    msgs = g(f"success_rec128_{n}.msgs").copy()
    offsets = np.arange(n + 1, dtype=np.uint64) * 156
    xid = (np.arange(n, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    spare = np.setdiff1d(np.arange(0x100, 0x400, dtype=np.uint32), xid)[:100]
    table_xids = np.sort(np.concatenate([xid[:200], spare]))  # sorted: the caller's order is the table's
    nc = table_xids.size
    p = R.PendingCalls(table_xids, 0, dev)
    plan, cp = M.Plan(S.rec128), compile_plan(S.rec128)
    st, od = to_dev(msgs, dev), u64_dev(offsets, dev)
    hdrs = torch.empty(n * A.RPC_HDR_BYTES, dtype=torch.uint8, device=dev)
    call = torch.empty(n, dtype=torch.int64, device=dev)
    reply_of = torch.empty(nc, dtype=torch.int64, device=dev)
    stats = torch.empty(nc, dtype=torch.int64, device=dev)
    kept = torch.empty(nc, dtype=torch.int64, device=dev)
    kept_pos = torch.empty(nc, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(A.lib().xdrg_rpc_pending_retire_workspace_size(nc), 16), dtype=torch.uint8, device=dev)

    def four(stream=None):
        R.launch_match_replies(st, od, p, hdrs, call, reply_of, stream)
        R.launch_verify_results(st, hdrs, call, p, [plan], 0, A.DEFAULT_STACK_LIMIT, None, stream)
        R.launch_call_stats(hdrs, reply_of, stats, A.RPCS_PENDING, stream)
        R.launch_pending_retire(p, reply_of, kept, kept_pos, count, ws, stream)

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
        if rnd == 1:  # 60 answered calls lose their reply (twice the same unknown xid), 50 of the others get one
            be = msgs.reshape(n, 156)
            assert 0xEE000001 not in table_xids
            be[:60, 4:8] = np.array([0xEE, 0, 0, 1], dtype=np.uint8)
            be[300:350, 4:8] = spare[:50].astype(">u4").view(np.uint8).reshape(50, 4)
            st.copy_(to_dev(msgs, dev))
        hdrs.copy_(R.check_replies(st, od))
        for t in (stats, kept, kept_pos, count, reply_of, call):
            t.fill_(-3)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want_h, want_call, want_reply, want_stats, (want_table, want_old, want_inv) = SM.settle(msgs, offsets, table_xids, 0, {0: cp})
        assert R.hdrs_numpy(hdrs).tobytes() == want_h.tobytes()
        assert np.array_equal(reply_of.cpu().numpy(), want_reply)
        assert np.array_equal(R.call_stats_numpy(stats), want_stats)
        k = int(count.item())
        assert k == len(want_table) and np.array_equal(kept[:k].cpu().numpy().view(R.CALL_DTYPE), want_table)
        want_pos = np.full(nc, -1, dtype=np.int64)
        want_pos[want_old] = want_inv
        assert np.array_equal(kept_pos.cpu().numpy(), want_pos)
        counts.append((k, int(np.count_nonzero(want_stats["type"] == A.RPCS_PENDING)),
                       int(np.count_nonzero(want_stats == np.array(SUCCESS, dtype=want_stats.dtype)))))
    assert counts == [(100, 100, 200), (110, 110, 190)]  # the replay followed the new bytes
