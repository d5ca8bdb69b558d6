"""GPU: xdrg_rpc_reply_batch (include/xdrgpu.h "Server reply batch"): the
success and error replies of a dispatched batch as the one ordered stream
srpc_server::run writes (xdrpp/srpc.cc:83-88).

Byte-exact against the numpy model of the contract (reply_stream_model.py),
which test_reply_batch_abi.py pins to the reference's own bytes; the golden
batch also against the stream assembled from those bytes without the model.
The copy of the emit kernel runs at both widths (16 bytes a lane, the
default, and 4 with XDRG_REPLY_BATCH_COPY=4) where the bytes are the point."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402
from xdrpp_amd.xdr_types import compile_plan  # noqa: E402
import oracle_bridge as O  # noqa: E402
import reply_stream_model as RS  # noqa: E402

ERROR_ACTIONS = (A.RPC_RPC_MISMATCH, A.RPC_PROG_UNAVAIL, A.RPC_PROG_MISMATCH, A.RPC_PROC_UNAVAIL,
                 A.RPC_GARBAGE_ARGS, A.RPC_SYSTEM_ERR, A.RPC_AUTH_ERROR)
GUARD = 64


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def u64_dev(a, dev):
    return to_dev(np.asarray(a, dtype=np.uint64).view(np.int64), dev)


def dev_source(s: RS.Src, dev) -> R.ResultSource:
    return R.ResultSource(u64_dev(s.index, dev),
                          None if s.xdr is None else to_dev(s.xdr, dev),
                          None if s.offsets is None else u64_dev(s.offsets, dev), s.fixed_size,
                          None if s.count is None else u64_dev([s.count], dev), len(s.index))


class Launch:
    """One raw xdrg_rpc_reply_batch call with everything it writes: the
    output with GUARD bytes of 0xA5 after its capacity, offsets, *d_unused
    and the status block."""

    def __init__(self, dev, hdrs: np.ndarray, sources, capacity: int):
        self.dev = dev
        self.n = len(hdrs)
        self.capacity = capacity
        self.hdrs = to_dev(np.ascontiguousarray(hdrs).view(np.uint8).reshape(-1), dev)
        self.sources = [s if isinstance(s, R.ResultSource) else dev_source(s, dev) for s in sources]
        self.buf = torch.full((capacity + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.offsets = torch.full((self.n + 1,), -1, dtype=torch.int64, device=dev)
        self.unused = torch.full((1,), -1, dtype=torch.int64, device=dev)
        self.status = M.Status(dev)
        need = A.lib().xdrg_rpc_reply_batch_workspace_size(self.n)
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    def launch(self, stream=None):
        R.launch_reply_batch(self.hdrs, self.sources, self.buf[:self.capacity], self.offsets, self.unused,
                             self.status, self.ws, stream)

    def read(self):
        """(stream, offsets, unused, err, total_bytes); the guard is checked."""
        e = self.status.read(M._stream())
        buf = self.buf.cpu().numpy()
        assert (buf[self.capacity:] == 0xA5).all(), "bytes written at or past out_capacity"
        offsets = self.offsets.cpu().numpy().view(np.uint64)
        err = (int(e.code), int(e.record)) if e.code else None
        upto = int(offsets[e.record]) if e.code else int(e.total_bytes)
        return buf[:min(upto, self.capacity)], offsets, int(self.unused.item()), err, int(e.total_bytes)


def run_and_compare(dev, hdrs, sources, capacity=None):
    """The device against the model: stream, offsets, total, *d_unused, error."""
    want, want_offs, want_unused, want_err = RS.model(hdrs, sources, capacity)
    cap = int(want_offs[-1]) if capacity is None else capacity
    c = Launch(dev, hdrs, sources, cap)
    c.status.init(M._stream())
    c.launch()
    stream, offsets, unused, err, total = c.read()
    assert np.array_equal(offsets, want_offs)
    assert total == int(want_offs[-1]) and unused == want_unused and err == want_err
    assert stream.tobytes() == want.tobytes()
    return stream, offsets


@pytest.fixture(params=[16, 4], ids=["copy16", "copy4"])
def width(request, monkeypatch):
    if request.param == 4:
        monkeypatch.setenv("XDRG_REPLY_BATCH_COPY", "4")
    else:
        monkeypatch.delenv("XDRG_REPLY_BATCH_COPY", raising=False)
    return request.param


@pytest.fixture(scope="module")
def batch():
    return RS.GoldenBatch()


# ------------------------------------------------------- reference bytes
def test_reference_error_replies(dev):
    hdrs = RS.g("rpccall_1024.hdrs").view(R.HDR_DTYPE)
    stream, offsets = run_and_compare(dev, hdrs, [])
    assert stream.tobytes() == RS.g("rpccall_1024.replies").tobytes()
    assert np.array_equal(offsets, RS.g("rpccall_1024.replyoffs", "<u8"))
    out, offs = R.reply_batch(to_dev(hdrs.view(np.uint8), dev), [])
    assert out.cpu().numpy().tobytes() == stream.tobytes()
    assert np.array_equal(offs.cpu().numpy().view(np.uint64), offsets)


def test_reference_success_replies(dev, width):
    n = 512
    msgs = RS.g("success_rec128_512.msgs")
    hdrs = np.zeros(n, dtype=R.HDR_DTYPE)
    hdrs["action"] = A.RPC_DISPATCH
    hdrs["xid"] = (np.arange(n, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    results = np.ascontiguousarray(msgs.reshape(n, 156)[:, 28:]).reshape(-1)
    stream, offsets = run_and_compare(dev, hdrs, [RS.Src(np.arange(n, dtype=np.uint64), results, None, 128)])
    assert stream.tobytes() == msgs.tobytes()
    assert np.array_equal(offsets, np.arange(n + 1, dtype=np.uint64) * 156)
    # the Python call, with the fixed size given and taken from the bytes
    for third in (128, None):
        out, offs = R.reply_batch(to_dev(hdrs.view(np.uint8), dev),
                                  [(u64_dev(np.arange(n), dev), to_dev(results, dev), third)])
        assert out.cpu().numpy().tobytes() == msgs.tobytes()


# ------------------------------------------------------ the golden batch
@pytest.mark.parametrize("layout", ["per_procedure", "per_type"])
def test_golden_batch(dev, batch, width, layout):
    """46 sources, one per served procedure, and three shuffled ones, one per
    result type: the same stream, the one assembled from the reference's
    bytes."""
    srcs = getattr(batch, layout)()
    assert len(srcs) == (46 if layout == "per_procedure" else 3)
    stream, offsets = run_and_compare(dev, batch.hdrs, srcs)
    want, want_offs = batch.expected()
    assert stream.tobytes() == want.tobytes() and np.array_equal(offsets, want_offs)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_golden_prefixes(dev, batch, n):
    stream, offsets = run_and_compare(dev, batch.hdrs[:n], batch.per_type(n))
    want, want_offs = batch.expected(n)
    assert stream.tobytes() == want.tobytes() and np.array_equal(offsets, want_offs)


def test_a_wave_that_writes_nothing(dev, batch, width):
    hdrs = batch.hdrs.copy()
    hdrs["action"][128:192] = A.RPC_DROP_NONCALL
    srcs = batch.per_type()
    stream, offsets = run_and_compare(dev, hdrs, srcs)
    assert offsets[128] == offsets[192]
    named = sum(int(np.count_nonzero((s.index >= 128) & (s.index < 192))) for s in srcs)
    assert named > 0 and RS.model(hdrs, srcs)[2] == named  # their entries are unused


def test_the_stream_reads_back(dev, batch):
    """The client's side of the result: index_messages finds the replies,
    check_replies classifies them."""
    hd = to_dev(batch.hdrs.view(np.uint8), dev)
    out, offs = R.reply_batch(hd, [(u64_dev(s.index, dev), None if s.xdr is None else to_dev(s.xdr, dev),
                                    s.fixed_size if s.offsets is None else u64_dev(s.offsets, dev))
                                   for s in batch.per_procedure()])
    offs = offs.cpu().numpy().view(np.uint64)
    replying = np.nonzero(np.diff(offs.astype(np.int64)) > 0)[0]
    ro = M.index_messages(out)
    assert np.array_equal(ro.cpu().numpy().view(np.uint64), np.append(offs[replying], offs[-1]))
    chk = R.hdrs_numpy(R.check_replies(out, ro))
    assert np.array_equal(chk["xid"], batch.hdrs["xid"][replying])
    success = batch.kind[replying] >= 0
    assert np.count_nonzero(success) == 201 + 213 + 176
    assert (chk["action"][success] == A.RPCR_OK).all() and (chk["err"] == 0).all()
    assert np.array_equal(chk["body_off"][success], offs[replying][success] + 28)
    assert np.array_equal(chk["end"], offs[replying + 1])
    # the rest: what the client makes of the reference's own error replies
    er = RS.g("rpccall_1024.replies")
    ero = RS.g("rpccall_1024.replyoffs", "<u8")
    ero = np.append(ero[:-1][np.diff(ero.astype(np.int64)) > 0], ero[-1])
    want = O.rpc_headers(er, ero, None, client=True)
    assert np.array_equal(chk["action"][~success], want["action"])
    assert np.array_equal(chk["w"][~success], want["w"])
    assert set(want["action"].tolist()) <= {A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH}


# ---------------------------------------------------------- long results
def test_long_results(dev, width):
    """16 void replies, two of them with 16,388 and 70,000 result bytes: one
    wave's stretch many rounds long, results past a lane's and a wave's
    step."""
    rng = np.random.default_rng(21)
    n = 16
    hdrs = np.zeros(n, dtype=R.HDR_DTYPE)
    hdrs["action"] = A.RPC_DISPATCH
    hdrs["xid"] = rng.integers(1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    sizes = np.zeros(n, dtype=np.uint64)
    sizes[3], sizes[9] = 16388, 70000
    xdr = rng.integers(256, size=int(sizes.sum()), dtype=np.uint8)
    src = RS.Src(np.arange(n, dtype=np.uint64), xdr, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    stream, offsets = run_and_compare(dev, hdrs, [src])
    assert stream.size == 28 * n + 16388 + 70000
    # the same bytes at every 4-byte alignment of the source run, behind 1..3 28-byte error replies
    for shift in (4, 8, 12):
        k = shift // 4
        h2 = np.concatenate([np.zeros(k, dtype=R.HDR_DTYPE), hdrs])
        h2["action"][:k] = A.RPC_GARBAGE_ARGS
        moved = RS.Src(src.index + np.uint64(k), np.concatenate([np.zeros(shift, dtype=np.uint8), xdr]),
                       src.offsets + np.uint64(shift))
        run_and_compare(dev, h2, [moved])


# ----------------------------------------------------------------- misuse
def small_batch():
    """24 messages: DISPATCH except 5 (GARBAGE_ARGS), 6 (DROP_NONCALL), 7
    (PROG_MISMATCH) and 20 (AUTH_ERROR)."""
    rng = np.random.default_rng(8)
    hdrs = np.zeros(24, dtype=R.HDR_DTYPE)
    hdrs["action"] = A.RPC_DISPATCH
    hdrs["xid"] = rng.integers(1 << 32, size=24, dtype=np.uint64).astype(np.uint32)
    hdrs["action"][[5, 6, 7, 20]] = [A.RPC_GARBAGE_ARGS, A.RPC_DROP_NONCALL, A.RPC_PROG_MISMATCH, A.RPC_AUTH_ERROR]
    hdrs["w"][7, A.RPC_W_LOW], hdrs["w"][7, A.RPC_W_HIGH] = 2, 9
    hdrs["w"][20, A.RPC_W_WHY] = 5
    return hdrs, rng


def test_two_sources_name_the_same_messages(dev):
    hdrs, rng = small_batch()
    idx = np.array([1, 2, 3, 4, 8, 9], dtype=np.uint64)
    a = RS.Src(idx, rng.integers(256, size=6 * 8, dtype=np.uint8), None, 8)
    b = RS.Src(idx[::-1].copy(), rng.integers(256, size=6 * 12, dtype=np.uint8), None, 12)
    for srcs, size in (([a, b], 8), ([b, a], 12)):  # the lower source wins
        stream, offsets = run_and_compare(dev, hdrs, srcs)
        assert int(offsets[2] - offsets[1]) == 28 + size
        assert RS.model(hdrs, srcs)[2] == 6
    # ... and inside one source the lower position
    twice = RS.Src(np.array([4, 4, 4], dtype=np.uint64), rng.integers(256, size=36, dtype=np.uint8),
                   np.array([0, 4, 16, 36], dtype=np.uint64))
    stream, offsets = run_and_compare(dev, hdrs, [twice])
    assert int(offsets[5] - offsets[4]) == 28 + 4 and RS.model(hdrs, [twice])[2] == 2


def test_unusable_entries(dev):
    hdrs, rng = small_batch()
    n = len(hdrs)
    xdr = rng.integers(256, size=256, dtype=np.uint8)
    # index = n and 2^63; an error, a dropped and an answered-by-header message
    idx = RS.Src(np.array([n, 1 << 63, 5, 6, 7, 20, 1], dtype=np.uint64), xdr, None, 16)
    # spans: past bytes_len, end < begin, offset 2 mod 4, length 2 mod 4, and one good
    spans = [RS.Src(np.array([k], dtype=np.uint64), xdr, np.array(ab, dtype=np.uint64))
             for k, ab in ((10, (248, 264)), (11, (40, 32)), (12, (42, 50)), (13, (40, 46)), (14, (24, 64)))]
    for srcs in ([idx], spans, [idx] + spans):
        run_and_compare(dev, hdrs, srcs)
    assert RS.model(hdrs, [idx])[2] == 6 and RS.model(hdrs, spans)[2] == 4


def test_device_count_below_the_cap(dev):
    hdrs, rng = small_batch()
    idx = np.array([1, 2, 3, 4, 8, 9, 10, 11], dtype=np.uint64)
    xdr = rng.integers(256, size=8 * 8, dtype=np.uint8)
    for count in (0, 3, 8, 100):
        srcs = [RS.Src(idx, xdr, None, 8, count), RS.Src(idx, None, None, 0, 5)]
        stream, offsets = run_and_compare(dev, hdrs, srcs)
        assert int(offsets[5] - offsets[4]) == 28 + (8 if count > 3 else 0)  # message 4: source 0 or the void one


# --------------------------------------------------------------- capacity
def test_capacity(dev, batch, width):
    srcs = batch.per_type()
    total = int(RS.model(batch.hdrs, srcs)[1][-1])
    want, want_offs, _, err = RS.model(batch.hdrs, srcs, total - 1)
    last = int(np.nonzero(np.diff(want_offs.astype(np.int64)) > 0)[0][-1])
    assert err == (A.ERR_OVERFLOW_PUT, last) and want.size == int(want_offs[last])
    run_and_compare(dev, batch.hdrs, srcs, total - 1)  # the guard after the capacity is checked there
    first = int(np.nonzero(np.diff(want_offs.astype(np.int64)) > 0)[0][0])
    assert RS.model(batch.hdrs, srcs, 0)[3] == (A.ERR_OVERFLOW_PUT, first)
    run_and_compare(dev, batch.hdrs, srcs, 0)
    run_and_compare(dev, batch.hdrs, srcs, total // 2)
    hd = to_dev(batch.hdrs.view(np.uint8), dev)
    ds = [dev_source(s, dev) for s in srcs]
    with pytest.raises(M.XdrRuntimeError) as ei:
        R.reply_batch(hd, ds, capacity=total - 1)
    assert ei.value.code == A.ERR_OVERFLOW_PUT and ei.value.record == last
    out, _ = R.reply_batch(hd, ds, capacity=total)  # exactly enough
    assert out.numel() == total
    out, _ = R.reply_batch(hd, ds)  # the default holds them
    assert out.numel() == total


# ------------------------------------------------------------- edge cases
def test_empty_batches(dev, batch):
    hdrs, rng = small_batch()
    none = np.zeros(0, dtype=R.HDR_DTYPE)
    idx = np.array([1, 2, 3], dtype=np.uint64)
    # n = 0: nothing written, every entry unused
    stream, offsets = run_and_compare(dev, none, [RS.Src(idx), RS.Src(idx, None, None, 0, 2)])
    assert stream.size == 0 and offsets.tolist() == [0]
    assert RS.model(none, [RS.Src(idx), RS.Src(idx, None, None, 0, 2)])[2] == 5
    run_and_compare(dev, none, [])
    # nsrcs = 0: the error replies alone
    stream, _ = run_and_compare(dev, hdrs, [])
    assert stream.size == 28 + 36 + 24
    # a source with no entries, by its cap and by its device count
    run_and_compare(dev, hdrs, [RS.Src(np.zeros(0, dtype=np.uint64)), RS.Src(idx)])
    run_and_compare(dev, hdrs, [RS.Src(idx, None, None, 0, 0), RS.Src(idx)])
    out, offs = R.reply_batch(torch.empty(0, dtype=torch.uint8, device=dev), [])
    assert out.numel() == 0 and offs.cpu().tolist() == [0]


# ---------------------------------------------------------- graph capture
def test_graph_capture(dev, batch):
    """One capture of launch_reply_batch on a single stream (kernels only, no
    parallel branches), replayed twice over changed result bytes, a changed
    action and a changed *d_count."""
    n = 256
    hdrs = batch.hdrs[:n].copy()
    srcs = batch.per_type(n)
    srcs[2] = srcs[2]._replace(count=len(srcs[2].index))  # the void source takes its count from the device
    total = int(RS.model(hdrs, srcs)[1][-1])
    c = Launch(dev, hdrs, srcs, total + 64)
    c.status.init(M._stream())
    c.launch()  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            c.launch(side.cuda_stream)
    victim = int(srcs[0].index[0])
    for rnd in range(2):
        if rnd == 1:  # new result bytes, one call fails after all, the void source is cut short
            srcs[0] = srcs[0]._replace(xdr=np.random.default_rng(rnd).integers(256, size=srcs[0].xdr.size,
                                                                               dtype=np.uint8))
            c.sources[0].xdr.copy_(to_dev(srcs[0].xdr, dev))
            hdrs["action"][victim] = A.RPC_SYSTEM_ERR
            c.hdrs.copy_(to_dev(hdrs.view(np.uint8).reshape(-1), dev))
            srcs[2] = srcs[2]._replace(count=7)
            c.sources[2].count.fill_(7)
        c.buf.fill_(0xA5)
        c.status.init(M._stream())
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want, want_offs, want_unused, _ = RS.model(hdrs, srcs)
        stream, offsets, unused, err, tot = c.read()
        assert err is None and tot == int(want_offs[-1]) and unused == want_unused
        assert np.array_equal(offsets, want_offs) and stream.tobytes() == want.tobytes()
    assert want_unused == 1  # the entry of the call that failed after all


# ------------------------------------------------------------- end to end
PROCS = {(100000, 2, 0): "rec128", (100000, 3, 1): "recvar", (100003, 3, 5): "containertest"}


def test_end_to_end_echo_server(dev):
    """index_messages -> dispatch -> decode_args -> (the handler echoes its
    argument) -> Marshaler.encode -> reply_batch, then the client's
    decode_results: every undamaged call gets its argument back, every
    damaged one GARBAGE_ARGS."""
    per = 256
    keys = list(PROCS)
    msgs, args = [], []
    for p, key in enumerate(keys):
        name = PROCS[key]
        cp = compile_plan(R.call_type(S.ALL[name]))
        nat, heap = W.GENERATORS[name](per)
        hdr = np.zeros((per, 10), dtype="<u4")
        hdr[:, 0] = ((np.arange(per, dtype=np.uint64) * 3 + p) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
        hdr[:, 2] = 2
        hdr[:, 3], hdr[:, 4], hdr[:, 5] = key
        rec = np.concatenate([hdr.view(np.uint8).reshape(per, 40), nat.reshape(per, cp.stride - 40)], axis=1)
        st, of = O.encode_msgs(cp, rec.reshape(-1), per, heap)
        msgs.append([st[int(of[i]):int(of[i + 1])] for i in range(per)])
    calls, xids, res, damaged = [], [], [], []
    for i in range(3 * per):  # the procedures in turn; every fifth call damaged
        m = msgs[i % 3][i // 3].copy()
        args.append(m[44:].copy())
        xids.append(int(m[4:8].view(">u4")[0]))
        res.append(i % 3)
        damaged.append(i % 5 == 0)
        if damaged[-1]:  # a word cut off the arguments, or one added
            body = m[4:-4] if (i // 5) % 2 else np.concatenate([m[4:], np.array([0xDEADBEEF], dtype=">u4").view(np.uint8)])
            m = np.concatenate([np.array([body.size | A.MARK_LAST], dtype=">u4").view(np.uint8), body])
        calls.append(m)
    damaged = np.array(damaged)
    assert len(set(xids)) == 3 * per
    # ---- the server
    st = to_dev(np.concatenate(calls), dev)
    hd = R.dispatch(st, M.index_messages(st), W.RPC_PROCS)
    plans = {key: M.Plan(S.ALL[name]) for key, name in PROCS.items()}
    decoded = R.decode_args(st, hd, plans)
    acts = R.hdrs_numpy(hd)["action"]
    assert (acts[damaged] == A.RPC_GARBAGE_ARGS).all() and (acts[~damaged] == A.RPC_DISPATCH).all()
    results = []
    for key in keys:
        index, native, heap = decoded[key]
        results.append((index, M.Marshaler(plans[key], dev).encode(native, index.numel(), heap)))
    replies, offs = R.reply_batch(hd, results)
    assert (np.diff(offs.cpu().numpy()) > 0).all()  # every call is answered, in call order
    # ---- the client
    pending = R.PendingCalls(np.array(xids, dtype=np.uint32), np.array(res, dtype=np.uint32), dev)
    ro = M.index_messages(replies)
    assert torch.equal(ro, offs)
    chd, call, reply_of, out = R.decode_results(replies, ro, pending, {p: plans[k] for p, k in enumerate(keys)})
    assert np.array_equal(call.cpu().numpy(), np.arange(3 * per)) and np.array_equal(reply_of.cpu().numpy(),
                                                                                     np.arange(3 * per))
    ch = R.hdrs_numpy(chd)
    assert (ch["action"][~damaged] == A.RPCR_OK).all()
    assert (ch["action"][damaged] == A.RPCR_ACCEPT_STAT).all() and (ch["w"][damaged, A.RPC_W_STAT] == 4).all()
    rb = replies.cpu().numpy()
    for i in np.nonzero(~damaged)[0]:
        assert rb[int(ch["body_off"][i]):int(ch["end"][i])].tobytes() == args[i].tobytes(), i
    index, native, _ = out[0]  # rec128: the decoded results are the generator's records
    want = W.rec128(per)[0].reshape(per, 128)
    assert np.array_equal(native.cpu().numpy().reshape(-1, 128), want[index.cpu().numpy() // 3])
