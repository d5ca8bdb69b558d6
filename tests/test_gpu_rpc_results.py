"""GPU: the asynchronous client's reply step for a batch
(xdrg_rpc_match_replies, xdrg_rpc_verify_results, xdrg_rpc_gather_results;
xdrpp/arpc.h:41-91, xdrpp/msgsock.cc:202-232): replies in any order are
joined to the pending calls by xid, the first reply to a call wins, every
matched reply's result is verified with its call's result type, and the
results left are gathered per type and decoded with the existing kernels.

Expected values: reply_model (the restatement's headers, a dict walked in
message order, the restatement's decode of each result slice), on the real
reference's bytes (tests/golden/success_rec128_512.msgs, rpc_1024.msgs) and
on the batches of reply_batches.  Integer work: compared exactly."""
import itertools
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
import oracle_bridge as O  # noqa: E402
import reply_batches as RB  # noqa: E402
import reply_model as RM  # noqa: E402
import verdict_model as V  # noqa: E402


def g(name, dtype=np.uint8):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def offs_dev(o, dev):
    return to_dev(np.asarray(o, dtype=np.uint64).view(np.int64), dev)


def same_hdrs(got: torch.Tensor, want: np.ndarray) -> bool:
    return R.hdrs_numpy(got).tobytes() == want.tobytes()


def match_and_compare(stream, offsets, xids, dev, res=0):
    """match_replies on the device == the model; returns both sides."""
    st, od = to_dev(stream, dev), offs_dev(offsets, dev)
    pending = R.PendingCalls(xids, res, dev)
    hd, call, reply_of = R.match_replies(st, od, pending)
    want_h, want_call, want_reply = RM.match(stream, offsets, xids)
    assert np.array_equal(call.cpu().numpy(), want_call)
    assert np.array_equal(reply_of.cpu().numpy(), want_reply)
    assert same_hdrs(hd, want_h)
    return st, od, pending, hd, call, (want_h, want_call, want_reply)


# ------------------------------------------------------- reference bytes
def test_reference_success_replies(dev):
    """The 512 success replies the real reference wrote (unique xids, one of
    them 0), the pending table all 512, shuffled: every reply matches, every
    verdict is 0, and decode_results equals Marshaler.decode of the results."""
    n = 512
    msgs = g(f"success_rec128_{n}.msgs")
    offsets = np.arange(n + 1, dtype=np.uint64) * 156
    xid = (np.arange(n, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    assert len(set(xid.tolist())) == n and xid[0] == 0 and msgs.size == 156 * n
    shuffle = np.random.default_rng(5).permutation(n)
    st, od, pending, hd, call, (want_h, want_call, want_reply) = match_and_compare(msgs, offsets, xid[shuffle], dev)
    assert np.array_equal(want_reply, shuffle) and (want_call >= 0).all()
    plan = M.Plan(S.rec128)
    v = R.verify_results(st, hd, call, pending, {0: plan})
    assert not v.cpu().numpy().any() and same_hdrs(hd, want_h)
    assert (R.hdrs_numpy(hd)["action"] == A.RPCR_OK).all()
    hd2, call2, reply2, out = R.decode_results(st, od, pending, {0: plan})
    assert same_hdrs(hd2, want_h) and np.array_equal(call2.cpu().numpy(), want_call)
    assert np.array_equal(reply2.cpu().numpy(), shuffle)
    index, native, _ = out[0]
    assert np.array_equal(index.cpu().numpy(), np.arange(n))
    results = np.ascontiguousarray(msgs.reshape(n, 156)[:, 28:]).reshape(-1)
    ref, _ = M.Marshaler(plan, dev).decode(to_dev(results, dev), n)
    assert torch.equal(native, ref)
    assert np.array_equal(native.cpu().numpy(), W.rec128(n)[0])


@pytest.mark.parametrize("result", ["void", "rec128"])
def test_all_reply_kinds(dev, result):
    """rpc_1024.msgs: 481 replies of every kind among 543 calls.  The
    pending table is every second reply's xid.  With a void
    result type the bodiless successes pass; with rec128 they become
    GARBAGE_RES (xdr_overflow)."""
    m, mo = g("rpc_1024.msgs"), g("rpc_1024.msgoffs", "<u8")
    n = mo.size - 1
    chk = g("rpc_1024.chk").view(R.HDR_DTYPE)
    words = np.array([[RM.be_word(m, int(mo[i]) + 4), RM.be_word(m, int(mo[i]) + 8)] if mo[i + 1] - mo[i] >= 12
                      else [0, 0xFFFFFFFF] for i in range(n)], dtype=np.uint64)
    replies = np.nonzero(words[:, 1] == 1)[0]
    assert replies.size == 481 and len(set(words[replies, 0].tolist())) == 481
    xids = words[replies[::2], 0].astype(np.uint32)
    st, od, pending, hd, call, (want_h, want_call, want_reply) = match_and_compare(m, mo, xids, dev)
    # the headers are the reference's own (rpc_1024.chk was written with the
    # synchronous client's xid test, which the join replaces: its BAD_XID
    # replies are OK here) with the model's rewrites
    expect = chk.copy()
    expect["action"][chk["action"] == A.RPCR_BAD_XID] = A.RPCR_OK
    unknown = want_h["action"] == A.RPCR_UNKNOWN_XID
    expect["action"][unknown] = A.RPCR_UNKNOWN_XID
    assert expect.tobytes() == want_h.tobytes() and np.count_nonzero(chk["action"] == A.RPCR_BAD_XID) == 11
    assert np.count_nonzero(want_h["action"] == A.RPCR_UNKNOWN_XID) == 240 and (want_reply >= 0).all()
    cp = None if result == "void" else compile_plan(S.rec128)
    plan = None if result == "void" else M.Plan(S.rec128)
    model = want_h.copy()
    want_v = RM.verify_results(m, model, want_call, np.zeros(xids.size, dtype=np.uint32), {0: cp})
    v = R.verify_results(st, hd, call, pending, {0: plan})
    assert np.array_equal(v.cpu().numpy().view(np.uint32), want_v)
    assert same_hdrs(hd, model)
    ok = (want_h["action"] == A.RPCR_OK) & (want_call >= 0)
    assert np.count_nonzero(ok) >= 16
    if result == "void":
        assert (model["action"][ok] == A.RPCR_OK).all() and not want_v[ok].any()
    else:
        assert (model["action"][ok] == A.RPCR_GARBAGE_RES).all() and (model["err"][ok] == A.ERR_OVERFLOW_GET).all()
    # matched error replies carry no result: untouched
    errs = np.isin(want_h["action"], (A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH)) & (want_call >= 0)
    assert np.count_nonzero(errs) >= 64 and not want_v[errs].any()
    for i in np.nonzero(model["action"] == A.RPCR_GARBAGE_RES)[0][:4]:
        assert R.call_stat_message(model[i]) == "unable to unmarshal reply value sent by server"


# ------------------------------------------------------ first reply wins
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_first_reply_wins(dev, n):
    stream, offsets, xids, xid_of = RB.first_reply_batch(n)
    st, od, pending, hd, call, (want_h, want_call, want_reply) = match_and_compare(stream, offsets, xids, dev)
    for a, b in [(a, b) for a, b in ((0, n - 1), (63, 64), (255, 256), (10, 20), (20, 30)) if a < b < n]:
        assert xid_of[a] == xid_of[b]
    first = {}
    for i, x in enumerate(xid_of.tolist()):  # the lowest message index of every xid wins
        if first.setdefault(x, i) == i:
            assert want_call[i] >= 0 and xids[want_call[i]] == x and want_reply[want_call[i]] == i
        else:
            assert want_call[i] == -1 and want_h["action"][i] == A.RPCR_UNKNOWN_XID
    assert np.count_nonzero(want_reply < 0) == n - len(first)  # the calls whose xid no message carries
    if n > 1:  # the malformed first copy wins and keeps its header
        assert want_h["action"][0] == A.RPCR_MALFORMED and want_call[0] >= 0 and len(first) < n
        assert want_call[n - 1] == -1  # its second copy
    v = R.verify_results(st, hd, call, pending, {0: None})
    model = want_h.copy()
    want_v = RM.verify_results(stream, model, want_call, np.zeros(n, dtype=np.uint32), {0: None})
    assert np.array_equal(v.cpu().numpy().view(np.uint32), want_v) and same_hdrs(hd, model)
    if n > 1:
        assert model["action"][0] == A.RPCR_GARBAGE_RES and model["err"][0] == A.ERR_BAD_DISCRIMINANT


# ----------------------------------------------------------- table edges
@pytest.mark.parametrize("ncalls", [0, 1, 2, 3])
def test_table_edges(dev, ncalls):
    """Tables of 0 to 3 calls drawn from the xids 0, 0x7fffffff, 0x80000000
    and 0xffffffff (the compare must be unsigned), in every order; no message
    answers 0x7fffffff."""
    pool = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    empty = np.zeros(0, dtype=np.uint8)
    msgs = [RB.success(x, empty) for x in (0xFFFFFFFF, 1, 0, 0x80000000, 0x80000001, 0, 0x7FFFFFFE)]
    msgs.insert(3, RB.message(RB.be_words([0x80000000, 0, 2, 1, 1, 1, 0, 0, 0, 0])))  # a CALL with a pending xid
    msgs.append(RB.message(RB.be_words([0])))  # too short to hold xid + msg_type
    stream, offsets = RB.stream_of(msgs)
    for xids in itertools.permutations(pool, ncalls):
        xids = np.array(xids, dtype=np.uint32)
        _, _, _, _, _, (want_h, want_call, want_reply) = match_and_compare(stream, offsets, xids, dev)
        for c, x in enumerate(xids):
            assert (want_reply[c] == -1) == (x == 0x7FFFFFFF)
        assert want_call[3] == -1 and want_h["action"][3] == A.RPCR_NOT_REPLY
        assert want_call[-1] == -1 and want_h["action"][-1] == A.RPCR_MALFORMED
        assert want_h["action"][6] == A.RPCR_UNKNOWN_XID  # the second reply to xid 0, pending or not


def test_empty_batches(dev):
    empty = torch.zeros(4, dtype=torch.uint8, device=dev)
    o = torch.zeros(1, dtype=torch.int64, device=dev)
    pending = R.PendingCalls([3, 1, 2], [0, 0, 0], dev)
    hd, call, reply_of = R.match_replies(empty, o, pending)
    assert hd.numel() == 0 and call.numel() == 0 and reply_of.cpu().tolist() == [-1, -1, -1]
    nobody = R.PendingCalls([], [], dev)
    hd, call, reply_of = R.match_replies(empty, o, nobody)
    assert hd.numel() == 0 and call.numel() == 0 and reply_of.numel() == 0
    assert R.verify_results(empty, hd, call, pending, {0: None}).numel() == 0
    data, offs, index = R.gather_results(empty, hd, call, pending, 0)
    assert data.numel() == 0 and index.numel() == 0 and offs.cpu().tolist() == [0]
    hd, call, reply_of, out = R.decode_results(empty, o, pending, {0: M.Plan(S.rec128), 1: None})
    assert out[0][0].numel() == 0 and out[1][0].numel() == 0 and reply_of.cpu().tolist() == [-1, -1, -1]


# ----------------------------------------------------------- mixed batch
@pytest.fixture(scope="module")
def batch():
    return RB.MixedBatch()


@pytest.fixture(scope="module")
def plans():
    return {r: None if name is None else M.Plan(S.ALL[name]) for r, name in RB.RES.items()}


@pytest.fixture()
def matched(batch, dev):
    """(stream, offsets, pending, matched headers, call) on the device."""
    st, od = to_dev(batch.stream, dev), offs_dev(batch.offsets, dev)
    pending = R.PendingCalls(batch.xids, batch.res, dev)
    hd, call, reply_of = R.match_replies(st, od, pending)
    assert np.array_equal(call.cpu().numpy(), batch.call)
    assert np.array_equal(reply_of.cpu().numpy(), batch.reply_of)
    assert same_hdrs(hd, batch.matched)
    return st, od, pending, hd, call


def test_mixed_match_touches_only_the_unknown(batch, matched):
    _, _, _, hd, _ = matched
    got = R.hdrs_numpy(hd)
    same = batch.matched["action"] != A.RPCR_UNKNOWN_XID
    assert got[same].tobytes() == batch.checked[same].tobytes()
    rest = batch.matched.copy()
    rest["action"] = batch.checked["action"]
    assert rest.tobytes() == batch.checked.tobytes()  # nothing but the action is rewritten


def test_mixed_verify_results(batch, plans, matched):
    st, _, pending, hd, call = matched
    v = R.verify_results(st, hd, call, pending, plans)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), batch.verdicts)
    assert same_hdrs(hd, batch.model)
    untouched = batch.verdicts == 0
    assert R.hdrs_numpy(hd)[untouched].tobytes() == batch.matched[untouched].tobytes()
    # a second pass finds nothing left to do
    assert not R.verify_results(st, hd, call, pending, plans).cpu().numpy().any()
    assert same_hdrs(hd, batch.model)


def test_mixed_verify_results_in_two_ranges(batch, plans, matched):
    """res_base: result types {0, 1} and {2, 3} in two calls == one call."""
    st, _, pending, hd, call = matched
    n = batch.call.size
    tcall = pending.to_table(call)
    v1 = torch.zeros(n, dtype=torch.int32, device=hd.device)
    v2 = torch.zeros(n, dtype=torch.int32, device=hd.device)
    R.launch_verify_results(st, hd, tcall, pending, [plans[2], plans[3]], 2, A.DEFAULT_STACK_LIMIT, v2)
    R.launch_verify_results(st, hd, tcall, pending, [plans[0], plans[1]], 0, A.DEFAULT_STACK_LIMIT, v1)
    r = np.where(batch.call >= 0, batch.res[np.clip(batch.call, 0, None)], 99)
    want1, want2 = np.where(r < 2, batch.verdicts, 0), np.where((r >= 2) & (r < 4), batch.verdicts, 0)
    assert np.array_equal(v1.cpu().numpy().view(np.uint32), want1)
    assert np.array_equal(v2.cpu().numpy().view(np.uint32), want2)
    assert same_hdrs(hd, batch.model)


def test_mixed_stack_limit_two(batch, plans, matched):
    """containertest results alone, stack limit 2."""
    st, _, pending, hd, call = matched
    model = batch.matched.copy()
    want = RM.verify_results(batch.stream, model, batch.call, batch.res, {2: batch.cps[2]}, stack_limit=2)
    assert np.count_nonzero(want & 0xFF == A.ERR_STACK_GET) >= 16
    v = R.verify_results(st, hd, call, pending, {2: plans[2]}, stack_limit=2)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), want)
    assert same_hdrs(hd, model)


def test_mixed_gather_results(batch, plans, matched):
    st, _, pending, hd, call = matched
    R.verify_results(st, hd, call, pending, plans)
    for r in list(RB.RES) + [RB.NO_PLAN_RES, 77]:
        want_idx = batch.selected(r)
        data, offs, index = R.gather_results(st, hd, call, pending, r)
        want_data, want_offs = RM.gathered(batch.slices(want_idx))
        assert np.array_equal(index.cpu().numpy(), want_idx), r
        assert np.array_equal(offs.cpu().numpy().view(np.uint64), want_offs), r
        assert data.cpu().numpy().tobytes() == want_data.tobytes(), r
    assert batch.selected(77).size == 0 and batch.selected(RB.NO_PLAN_RES).size >= 32


def test_mixed_gather_capacity(batch, plans, matched):
    st, _, pending, hd, call = matched
    R.verify_results(st, hd, call, pending, plans)
    idx = batch.selected(1)
    ends = np.cumsum([p.size for p in batch.slices(idx)])
    total = int(ends[-1])
    data, _, _ = R.gather_results(st, hd, call, pending, 1, capacity=total)  # exactly enough
    assert data.numel() == total
    for cap in (total - 1, total // 2):
        with pytest.raises(M.XdrRuntimeError) as ei:
            R.gather_results(st, hd, call, pending, 1, capacity=cap)
        assert ei.value.code == A.ERR_OVERFLOW_PUT and ei.value.record == idx[np.nonzero(ends > cap)[0][0]]


def test_mixed_decode_results(batch, plans, dev):
    st, od = to_dev(batch.stream, dev), offs_dev(batch.offsets, dev)
    pending = R.PendingCalls(batch.xids, batch.res, dev)
    hd, call, reply_of, out = R.decode_results(st, od, pending, plans)
    assert same_hdrs(hd, batch.model)
    assert np.array_equal(call.cpu().numpy(), batch.call)
    assert np.array_equal(reply_of.cpu().numpy(), batch.reply_of)
    assert sorted(out) == sorted(RB.RES)
    for r, (index, native, heap) in out.items():
        want_idx = batch.selected(r)
        assert np.array_equal(index.cpu().numpy(), want_idx)
        if batch.cps[r] is None:
            assert native is None and heap is None
            continue
        data, offs = RM.gathered(batch.slices(want_idx))
        o_nat, o_heap = O.decode(batch.cps[r], data, len(want_idx), offs)  # no error: they were verified
        assert np.array_equal(native.cpu().numpy(), o_nat), r
        if not plans[r].is_fixed:
            assert np.array_equal(heap.cpu().numpy(), o_heap), r


# --------------------------------------------------------- graph capture
def test_graph_capture_replays_follow_the_data(dev):
    """check + match + verify captured once and replayed over a stream that
    changes between replays: headers, call, reply_of and verdicts follow the
    data (reply_of is filled again by every replay)."""
    n = 300
    cp = compile_plan(S.recvar)
    plan = M.Plan(S.recvar)
    nat, heap = W.recvar(n)
    x, ro = O.encode(cp, nat, n, heap)
    rng = np.random.default_rng(9)
    xids = RB.unique_xids(rng, n + 8)
    msgs = [RB.success(int(xids[i]), x[int(ro[i]):int(ro[i + 1])]) for i in range(n)]
    stream, offsets = RB.stream_of(msgs)
    pending = R.PendingCalls(xids, 0, dev)  # 8 calls are never answered
    st, od = to_dev(stream, dev), offs_dev(offsets, dev)
    hd = torch.zeros(n * A.RPC_HDR_BYTES, dtype=torch.uint8, device=dev)
    tcall = torch.zeros(n, dtype=torch.int64, device=dev)
    treply = torch.zeros(pending.ncalls, dtype=torch.int64, device=dev)
    verdicts = torch.zeros(n, dtype=torch.int32, device=dev)

    def launch(s):
        A.check(A.lib().xdrg_rpc_check_replies(st.data_ptr(), st.numel(), od.data_ptr(), n, None, hd.data_ptr(), s),
                "xdrg_rpc_check_replies")
        R.launch_match_replies(st, od, pending, hd, tcall, treply, stream=s)
        R.launch_verify_results(st, hd, tcall, pending, [plan], 0, A.DEFAULT_STACK_LIMIT, verdicts, stream=s)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm: the plan's tables outside the capture
        launch(side.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(torch.cuda.current_stream().cuda_stream)
    perm, inv = pending.perm.cpu().numpy(), pending.inv.cpu().numpy()
    s2 = stream.copy()
    for damaged, strangers in (([], []), ([5, 64, 299], [7]), ([5, 64, 299], [7]), ([7], [0, 128]), ([], [])):
        s2[:] = stream
        for r in damaged:
            V.put_be(s2, int(offsets[r]) + 28 + 12, 0xFFFFFFFF)  # the result's opaque blob<256> length word
        for r in strangers:
            V.put_be(s2, int(offsets[r]) + 4, int(xids[r]) ^ 0x55555555)  # an xid nobody waits for
        st.copy_(to_dev(s2, dev))
        hd.fill_(0xEE)
        tcall.fill_(12345)
        treply.fill_(12345)
        verdicts.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        model, want_call, want_reply = RM.match(s2, offsets, xids)
        want_v = RM.verify_results(s2, model, want_call, np.zeros(xids.size, dtype=np.uint32), {0: cp})
        assert sorted(np.nonzero(model["action"] == A.RPCR_UNKNOWN_XID)[0]) == sorted(strangers)
        assert sorted(np.nonzero(want_v)[0]) == sorted(set(damaged) - set(strangers))
        got_call = tcall.cpu().numpy()
        assert np.array_equal(np.where(got_call >= 0, perm[np.clip(got_call, 0, None)], got_call), want_call)
        assert np.array_equal(treply.cpu().numpy()[inv], want_reply)
        assert np.array_equal(verdicts.cpu().numpy().view(np.uint32), want_v)
        assert same_hdrs(hd, model)


# ------------------------------------------------------------ round trip
def test_round_trip_through_both_halves(dev):
    """192 calls through the server half and back through the client half, on
    the device: call_type encode, index_messages, dispatch, decode_args, the
    arguments echoed as results through success_reply_type with the xids of
    the headers, error_replies appended, decode_results.  Every intact call's
    result equals its arguments; every damaged call comes back ACCEPT_STAT /
    GARBAGE_ARGS."""
    n = 192
    key = tuple(int(v) for v in W.RPC_PROCS[W.RPC_PROCS[:, 3] == 0][5][:3])
    arg_plan = M.Plan(S.recvar)
    # (the interpreting kernels: no plan-specialized compile for two plans only this test has)
    call_plan = M.Plan(R.call_type(S.recvar), {"specialize": 0})
    reply_plan = M.Plan(R.success_reply_type(S.recvar), {"specialize": 0})
    stride = arg_plan.stride
    assert call_plan.stride == 40 + stride and reply_plan.stride == 24 + stride
    args, heap = W.recvar(n)
    xid = (np.arange(n, dtype=np.uint64) * 2654435761 + 17 & 0xFFFFFFFF).astype(np.uint32)
    hdr = np.zeros((n, 10), dtype="<u4")
    hdr[:, 0], hdr[:, 2] = xid, 2
    hdr[:, 3], hdr[:, 4], hdr[:, 5] = key
    nat = np.concatenate([hdr.view(np.uint8).reshape(n, 40), args.reshape(n, stride)], axis=1).reshape(-1)
    d_heap = to_dev(heap, dev)
    calls = M.Marshaler(call_plan, dev).encode_msgs(to_dev(nat, dev), n, d_heap)
    st = calls.xdr
    damaged = np.arange(3, n, 7)
    marks = calls.offsets.cpu().numpy()
    for r in damaged:  # the argument's opaque blob<256> length word
        st[int(marks[r]) + 44 + 12:int(marks[r]) + 44 + 16] = 0xFF
    # the server half
    offs = M.index_messages(st)
    assert np.array_equal(offs.cpu().numpy(), marks)
    hd = R.dispatch(st, offs, W.RPC_PROCS)
    index, a_nat, a_heap = R.decode_args(st, hd, {key: arg_plan})[key]
    intact = np.setdiff1d(np.arange(n), damaged)
    assert np.array_equal(index.cpu().numpy(), intact)
    k = index.numel()
    reply_nat = torch.zeros((k, 24 + stride), dtype=torch.uint8, device=dev)
    words = torch.zeros((k, 6), dtype=torch.int32, device=dev)
    words[:, 0] = hd.view(torch.int32).reshape(n, 16)[index, 0]  # the xids, from the headers
    words[:, 1] = 1
    reply_nat[:, :24] = words.view(torch.uint8)
    reply_nat[:, 24:] = a_nat.reshape(k, stride)
    good = M.Marshaler(reply_plan, dev).encode_msgs(reply_nat.reshape(-1), k, a_heap)
    bad, _ = R.error_replies(hd)
    back = torch.cat([good.xdr, bad])
    # the client half
    pending = R.PendingCalls(xid, 0, dev)
    hdrs, call, reply_of, out = R.decode_results(back, M.index_messages(back), pending, {0: arg_plan})
    h, call, reply_of = R.hdrs_numpy(hdrs), call.cpu().numpy(), reply_of.cpu().numpy()
    assert h.size == n and (reply_of >= 0).all() and sorted(call.tolist()) == list(range(n))
    assert (h["action"][reply_of[intact]] == A.RPCR_OK).all()
    assert (h["action"][reply_of[damaged]] == A.RPCR_ACCEPT_STAT).all()
    assert (h["w"][reply_of[damaged], A.RPC_W_STAT] == 4).all()  # GARBAGE_ARGS
    assert R.call_stat_message(h[reply_of[damaged[0]]]) == "procedure can't decode params"
    r_index, r_nat, r_heap = out[0]
    whose = call[r_index.cpu().numpy()]  # the call each decoded result answers
    assert np.array_equal(np.sort(whose), intact)
    # results == arguments: re-encoded, they are the arguments' own XDR
    again = M.Marshaler(arg_plan, dev).encode(r_nat, r_index.numel(), r_heap)
    cp = compile_plan(S.recvar)
    want, wo = O.encode(cp, args, n, heap)
    pieces = [want[int(wo[c]):int(wo[c + 1])] for c in whose]
    assert again.xdr.cpu().numpy().tobytes() == np.concatenate(pieces).tobytes()
