"""GPU: the carry between the rounds of the tile scan (k_tile_scan,
xdrpp_amd/csrc/batch_kernels.h) in the four calls whose own suites stop at
1,024 messages: xdrg_rpc_reply_batch, xdrg_rpc_call_batch,
xdrg_rpc_gather_args and xdrg_rpc_gather_results.  (The settle tests reach it
at TILE * SCAN_LANES + 1 entries.)

N = 256 * 1024 + 1 messages is the smallest batch whose 1,025 tiles need a
second round.  The payloads are void or 8 bytes, so the streams stay at a few
MB.  Offsets, totals, counts and index are computed here in numpy from the
contract; the output bytes of the last two tiles (messages TAIL onward) are
compared with the stage's model run on that sub-batch -- a message's bytes
depend on its own header and its winning entry alone -- or, for the gathers,
with the bodies sliced from the input stream."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
import call_stream_model as CS  # noqa: E402
import reply_stream_model as RS  # noqa: E402

TILE, SCAN_LANES = 256, 1024
N = TILE * SCAN_LANES + 1
TAIL = N - TILE - 1  # 261,888: the first message of the last two tiles
GUARD = 64


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def u64_dev(a, dev):
    return to_dev(np.asarray(a, dtype=np.uint64).view(np.int64), dev)


def cumsum0(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)


def payload(msgs) -> np.ndarray:
    """8 bytes per message that name it: the message number, big-endian."""
    return np.asarray(msgs).astype(">u8").view(np.uint8).reshape(-1)


def tail_of(index: np.ndarray, xdr8: bool):
    """The entries of a source that name messages from TAIL on, re-based:
    (index, xdr) -- an entry's 8 bytes travel with it."""
    keep = index >= TAIL
    idx = (index[keep] - TAIL).astype(np.uint64)
    return idx, (payload(index[keep]) if xdr8 else None)


# ------------------------------------------------------------ reply stream
def test_reply_batch_second_round(dev):
    rng = np.random.default_rng(7)
    hdrs = np.zeros(N, dtype=R.HDR_DTYPE)
    hdrs["action"] = A.RPC_DISPATCH
    hdrs["xid"] = (np.arange(N, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    hdrs["action"][0] = A.RPC_PROG_MISMATCH
    hdrs["w"][0, A.RPC_W_LOW], hdrs["w"][0, A.RPC_W_HIGH] = 2, 5
    hdrs["action"][N - 2] = A.RPC_AUTH_ERROR
    hdrs["w"][N - 2, A.RPC_W_WHY] = 3
    hdrs["action"][N - 1] = A.RPC_RPC_MISMATCH
    served = hdrs["action"] == A.RPC_DISPATCH
    kind = np.arange(N) % 3  # 0: an 8-byte result, 1: a void result, 2: not answered yet
    fixed_idx = rng.permutation(np.nonzero(served & (kind == 0))[0]).astype(np.uint64)
    void_msgs = np.nonzero(served & (kind == 1))[0]
    # four entries that win nothing: two name error replies, one no message, one a message already won
    void_idx = np.concatenate([void_msgs, [0, N - 1, N + 5, void_msgs[-1]]]).astype(np.uint64)

    sizes = np.zeros(N, dtype=np.uint64)
    sizes[served & (kind == 0)] = 28 + 8
    sizes[served & (kind == 1)] = 28
    sizes[0], sizes[N - 2], sizes[N - 1] = 36, 24, 28  # PROG_MISMATCH, AUTH_ERROR, RPC_MISMATCH (server.cc:8-67)
    want_offs = cumsum0(sizes)
    total = int(want_offs[-1])

    srcs = [R.ResultSource(u64_dev(fixed_idx, dev), to_dev(payload(fixed_idx), dev), None, 8),
            R.ResultSource(u64_dev(void_idx, dev))]
    buf = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    offsets = torch.full((N + 1,), -1, dtype=torch.int64, device=dev)
    unused = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(A.lib().xdrg_rpc_reply_batch_workspace_size(N), dtype=torch.uint8, device=dev)
    st = M.Status(dev)
    st.init(M._stream())
    R.launch_reply_batch(to_dev(hdrs.view(np.uint8).reshape(-1), dev), srcs, buf[:total], offsets, unused, st, ws)
    e = st.read(M._stream())
    assert e.code == 0 and int(e.total_bytes) == total
    assert np.array_equal(offsets.cpu().numpy().view(np.uint64), want_offs)
    assert int(unused.item()) == 4
    out = buf.cpu().numpy()
    assert (out[total:] == 0xA5).all(), "bytes written at or past out_capacity"

    sub = [RS.Src(*tail_of(fixed_idx, True), None, 8), RS.Src(*tail_of(void_idx, False))]
    want, sub_offs, _, err = RS.model(hdrs[TAIL:], sub)
    assert err is None and np.array_equal(sub_offs, want_offs[TAIL:] - want_offs[TAIL])
    assert out[int(want_offs[TAIL]):total].tobytes() == want.tobytes()


# ------------------------------------------------------------- call stream
def test_call_batch_second_round(dev):
    rng = np.random.default_rng(8)
    xids = (np.arange(N, dtype=np.uint64) + 0xFFFF0000 & 0xFFFFFFFF).astype(np.uint32)  # they wrap on the way
    kind = np.arange(N) % 3  # 0: 8 bytes of arguments, 1: none, 2: no entry (unsent)
    key8, key0 = (100003, 4, 17), (100003, 4, 18)
    fixed_idx = rng.permutation(np.nonzero(kind == 0)[0]).astype(np.uint64)
    void_calls = np.nonzero(kind == 1)[0]
    # two entries that win nothing: one names no position, one a position already won
    void_idx = np.concatenate([void_calls, [N + 3, void_calls[0]]]).astype(np.uint64)

    sizes = np.where(kind == 0, 44 + 8, np.where(kind == 1, 44, 0)).astype(np.uint64)
    want_offs = cumsum0(sizes)
    total = int(want_offs[-1])
    want_sent = np.zeros(N, dtype=R.CALL_DTYPE)
    want_sent["xid"] = xids
    want_sent["res"] = np.where(kind == 0, 1, np.where(kind == 1, 2, A.RPC_RES_UNSENT))

    srcs = [R.ArgSource(key8, 1, u64_dev(fixed_idx, dev), to_dev(payload(fixed_idx), dev), None, 8),
            R.ArgSource(key0, 2, u64_dev(void_idx, dev))]
    buf = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    offsets = torch.full((N + 1,), -1, dtype=torch.int64, device=dev)
    sent = torch.full((N,), -1, dtype=torch.int64, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(A.lib().xdrg_rpc_call_batch_workspace_size(N), dtype=torch.uint8, device=dev)
    st = M.Status(dev)
    st.init(M._stream())
    R.launch_call_batch(to_dev(xids.view(np.int32), dev), srcs, buf[:total], offsets, sent, counts, st, ws)
    e = st.read(M._stream())
    assert e.code == 0 and int(e.total_bytes) == total
    assert np.array_equal(offsets.cpu().numpy().view(np.uint64), want_offs)
    assert counts.cpu().tolist() == [int((kind == 2).sum()), 2]
    assert np.array_equal(sent.cpu().numpy().view(R.CALL_DTYPE), want_sent)
    out = buf.cpu().numpy()
    assert (out[total:] == 0xA5).all(), "bytes written at or past out_capacity"

    sub = [CS.Src(key8, 1, *tail_of(fixed_idx, True), None, 8), CS.Src(key0, 2, *tail_of(void_idx, False))]
    want, sub_offs, _, _, err = CS.model(xids[TAIL:], sub)
    assert err is None and np.array_equal(sub_offs, want_offs[TAIL:] - want_offs[TAIL])
    assert out[int(want_offs[TAIL]):total].tobytes() == want.tobytes()


# ----------------------------------------------------------------- gathers
def gather_batch(ok_action: int):
    """N headers over a stream of 8 bytes a message: message i's body is its
    own 8 bytes when i is even, empty when odd.  Messages 0, N - 3 and N - 2
    carry another action; message N - 1, alone in the one tile of the scan's
    second round, keeps the selected action and (N - 1 is even) a body, so its
    index, offset and bytes depend on that round's bases."""
    stream = payload(np.arange(N))
    hdrs = np.zeros(N, dtype=R.HDR_DTYPE)
    hdrs["action"] = ok_action
    hdrs["action"][[0, N - 3, N - 2]] = ok_action + 1
    at = 8 * np.arange(N, dtype=np.uint64)
    hdrs["body_off"] = at
    hdrs["end"] = at + np.where(np.arange(N) % 2 == 0, 8, 0).astype(np.uint64)
    return stream, hdrs


def check_gather(dev, call, stream, hdrs, selected):
    """Runs one gather (call(ptrs...) launches it) and checks everything it
    writes against the selection."""
    assert selected[N - 1] and hdrs["end"][N - 1] - hdrs["body_off"][N - 1] == 8, "the second round's tile is empty"
    want_index = np.nonzero(selected)[0].astype(np.uint64)
    count = want_index.size
    sizes = (hdrs["end"] - hdrs["body_off"])[selected]
    want_offs = cumsum0(sizes)
    total = int(want_offs[-1])
    body = (np.arange(N) % 2 == 0) & selected
    want = stream.reshape(N, 8)[body].reshape(-1)
    assert want.size == total

    out = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    offs = torch.full((N + 1,), -1, dtype=torch.int64, device=dev)
    index = torch.full((N,), -1, dtype=torch.int64, device=dev)
    cnt = torch.full((1,), -1, dtype=torch.int64, device=dev)
    st = M.Status(dev)
    st.init(M._stream())
    call(to_dev(stream, dev), to_dev(hdrs.view(np.uint8).reshape(-1), dev), out, total, offs, index, cnt, st)
    e = st.read(M._stream())
    assert e.code == 0 and int(e.total_bytes) == total
    assert int(cnt.item()) == count
    assert np.array_equal(offs.cpu().numpy().view(np.uint64)[:count + 1], want_offs)
    assert np.array_equal(index.cpu().numpy().view(np.uint64)[:count], want_index)
    got = out.cpu().numpy()
    assert (got[total:] == 0xA5).all(), "bytes written at or past the capacity"
    k0 = int(np.searchsorted(want_index, TAIL))  # the first selected message of the last two tiles
    assert count - k0 > TILE // 4
    assert got[int(want_offs[k0]):total].tobytes() == want[int(want_offs[k0]):].tobytes()
    assert got[:total].tobytes() == want.tobytes()


def test_gather_args_second_round(dev):
    stream, hdrs = gather_batch(A.RPC_DISPATCH)
    key = (100003, 4, 17)
    hdrs["w"][:, A.RPC_W_PROG], hdrs["w"][:, A.RPC_W_VERS] = key[0], key[1]
    hdrs["w"][:, A.RPC_W_PROC] = np.where(np.arange(N) % 3 == 2, key[2] + 1, key[2])  # every third: another procedure
    selected = (hdrs["action"] == A.RPC_DISPATCH) & (np.arange(N) % 3 != 2)
    L = A.lib()
    ws = torch.empty(L.xdrg_rpc_gather_workspace_size(N), dtype=torch.uint8, device=dev)

    def call(s, h, out, cap, offs, index, cnt, st):
        A.check(L.xdrg_rpc_gather_args(M._ptr(s), s.numel(), M._ptr(h), N, *key, out.data_ptr(), cap, offs.data_ptr(),
                                       index.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), st.ptr,
                                       M._stream()), "xdrg_rpc_gather_args")

    check_gather(dev, call, stream, hdrs, selected)


def test_gather_results_second_round(dev):
    stream, hdrs = gather_batch(A.RPCR_OK)
    table = np.zeros(4, dtype=R.CALL_DTYPE)
    table["xid"], table["res"] = [10, 20, 30, 40], [5, 7, 5, 9]
    call_of = (np.arange(N) % 5).astype(np.uint64)  # 4: no entry of the table
    call_of[np.arange(N) % 35 == 0] = A.RPC_NO_CALL
    call_of[N - 1] = 2  # the message of the second round's tile is selected
    selected = (hdrs["action"] == A.RPCR_OK) & np.isin(call_of, [0, 2])  # the calls with res == 5
    L = A.lib()
    ws = torch.empty(L.xdrg_rpc_gather_results_workspace_size(N), dtype=torch.uint8, device=dev)
    t_call, t_table = u64_dev(call_of, dev), to_dev(table.view(np.int64), dev)

    def call(s, h, out, cap, offs, index, cnt, st):
        A.check(L.xdrg_rpc_gather_results(M._ptr(s), s.numel(), M._ptr(h), M._ptr(t_call), N, M._ptr(t_table), 4, 5,
                                          out.data_ptr(), cap, offs.data_ptr(), index.data_ptr(), cnt.data_ptr(),
                                          ws.data_ptr(), ws.numel(), st.ptr, M._stream()),
                "xdrg_rpc_gather_results")

    check_gather(dev, call, stream, hdrs, selected)
