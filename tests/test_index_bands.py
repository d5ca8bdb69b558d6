"""The record index and the message index at the lengths the speculative
walk's geometry turns on (xdrpp_amd/csrc/index_kernels.h rxs_walk / rxs_check /
rxs_fix / rxs_emit, run_index and rx_windows in xdrgpu.hip): records and
messages between one lane and one index window, which the streams of
tests/test_record_index.py (records under 1 KB, or 16-80 KiB) do not hold.

The streams are written by hand here, so their offsets are the ground
truth: the CPU half checks that the C restatement (oracle/xdr_oracle.c)
walks every good stream to exactly those offsets, and the GPU half then
compares the device with the restatement on the good and the damaged
streams -- offsets, count, error code and the error's record, all exact.
"""
import functools
import time

import numpy as np
import pytest

from xdrpp_amd import _abi as A
from xdrpp_amd.xdr_types import compile_plan
import oracle_bridge as O
from test_long_messages import device_index
from test_record_index import _dev, _fast_flag, _gpu_index, bigrec_type, damaged, tiled

# The walk's geometry (index_kernels.h); the bands below follow from it.
SUB = 124                  # kRxsSub: bytes per lane
BACK = 8 * SUB             # kRxsBack: the look-back, lanes 0-7
SEG = 64 * SUB - BACK      # kRxsSeg: bytes per segment (one wave)
AHEAD = 9 * 1024 - 64 * SUB  # kRxsAhead: staged past the segment
STG = BACK + SEG + AHEAD   # the staged stretch
WALK_MIN = 4 * SEG         # run_index walks from this length on

BANDS = [
    124,    # kRxsSub: one lane
    992,    # kRxsBack: the look-back
    1280,   # kRxsAhead: staged after the segment
    2272,   # kRxsBack + kRxsAhead: from the look-back's start past a lane-sized segment rest
    6944,   # kRxsSeg: one segment
    7936,   # kRxsSeg + kRxsBack: starts in the look-back and spans the segment
    9216,   # the staged stretch (kRxsBack + kRxsSeg + kRxsAhead)
    13888,  # 2 * kRxsSeg: an exit that passes over a whole segment
    16380,  # XDRG_INDEX_MAX_MSG: the index window
]
KINDS = ["random", "zeros", "nested", "tail"]
MODES = ["windowed", "whole"]
TOTAL = 1 << 18  # bytes per stream, at least (about 37 segments)


def test_geometry():
    assert (SUB, BACK, AHEAD, SEG, STG) == (124, 992, 1280, 6944, 9216)
    assert BANDS == [SUB, BACK, AHEAD, BACK + AHEAD, SEG, SEG + BACK, STG, 2 * SEG, A.INDEX_MAX_MSG]
    assert WALK_MIN == 27776


def _pad(b):
    return b + b"\0" * (-len(b) % 4)


def rec(i, blob, name):
    """One bigrec record on the wire."""
    return (int(i).to_bytes(8, "big") + len(blob).to_bytes(4, "big") + _pad(blob)
            + len(name).to_bytes(4, "big") + _pad(name))


def _rand(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def payload(kind, n, rng, band):
    """n blob bytes.  random: guesses inside break.  zeros: every word starts
    a chain of 16-byte records (7 nodes a lane, past kRxsKeep).  nested:
    well-formed records with blobs of 0-300 bytes, cut at n (chains with real
    jumps, some past the record's end).  tail (band records; random
    elsewhere): random bytes whose last 16 k bytes are zeros, k in 1..8 -- a
    chain of 16-byte records up to the blob's end, which lands on the
    name-length word or 4 / 8 / 12 bytes off it."""
    if kind == "zeros":
        return bytes(n)
    if kind == "nested":
        out = b""
        while len(out) < n:
            out += rec(int(rng.integers(0, 2**40)), _rand(rng, int(rng.integers(0, 300))), b"ab")
        return out[:n]
    if kind == "tail" and band:
        z = min(16 * int(rng.integers(1, 9)), n & ~15)
        return _rand(rng, n - z) + bytes(z)
    return _rand(rng, n)


def _offsets(recs):
    offs = np.zeros(len(recs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(w) for w in recs])
    return np.frombuffer(b"".join(recs), dtype=np.uint8).copy(), offs, len(recs)


@functools.lru_cache(maxsize=None)
def band_stream(B, kind, clamp):
    """(stream, offsets, n): about one record in three B - 4, B or B + 4
    bytes long (at most clamp), its blob sized for that and its name 0, 4 or
    8 bytes; the rest short (a blob under 200 bytes, a name up to 64), which
    shift the band records against the segment grid."""
    rng = np.random.default_rng(1000 * B + KINDS.index(kind))
    out, size, i = [], 0, 0
    while size < TOTAL:
        if rng.integers(0, 3) == 0:
            L = min(B + 4 * int(rng.integers(-1, 2)), clamp)
            nl = 4 * int(rng.integers(0, 3))
            r = rec(i, payload(kind, L - 16 - nl, rng, True), b"n" * nl)
            assert len(r) == L
        else:
            r = rec(i, payload(kind, int(rng.integers(0, 200)), rng, False),
                    bytes(rng.integers(97, 123, int(rng.integers(0, 65)), dtype=np.uint8)))
        out.append(r)
        size += len(r)
        i += 1
    return _offsets(out)


def mode_stream(B, kind, mode):
    """The band's stream and the mode's max_rec_len: the windowed index takes
    records up to the window, so its stream's records stop there."""
    if mode == "windowed":
        return band_stream(B, kind, A.INDEX_MAX_MSG) + (A.INDEX_MAX_MSG,)
    return band_stream(B, kind, 1 << 30) + (A.MAX_MSG,)


@functools.lru_cache(maxsize=None)
def past_window_stream():
    """Short records around one of 16384 bytes, 4 past the window."""
    rng = np.random.default_rng(77)
    out = [rec(i, _rand(rng, int(rng.integers(0, 200))), b"nm") for i in range(600)]
    at = 311
    out[at] = rec(at, _rand(rng, 16384 - 16), b"")
    assert len(out[at]) == A.INDEX_MAX_MSG + 4
    return _offsets(out) + (at,)


@functools.lru_cache(maxsize=None)
def _cp():
    return compile_plan(bigrec_type())


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", BANDS)
def test_oracle_walks_the_band_streams(B, kind, mode):
    """The restatement gives the constructed offsets: they are the truth the
    device is held to."""
    x, offs, n, maxlen = mode_stream(B, kind, mode)
    sizes = np.diff(offs.astype(np.int64))
    assert x.size >= TOTAL >= WALK_MIN
    assert {B - 4, B, min(B + 4, maxlen)} <= set(sizes.tolist()) and sizes.max() <= max(B + 4, 284)
    got, cnt, rc, _ = O.index_records(_cp(), x, n, maxlen)
    assert rc == 0 and cnt == n and np.array_equal(got, offs)


def test_oracle_past_window_record():
    x, offs, n, at = past_window_stream()
    assert x.size >= WALK_MIN
    got, cnt, rc, er = O.index_records(_cp(), x, n, A.INDEX_MAX_MSG)
    assert rc == A.ERR_INDEX_LONG and er == at and np.array_equal(got[:at + 1], offs[:at + 1])
    got, cnt, rc, _ = O.index_records(_cp(), x, n, A.MAX_MSG)
    assert rc == 0 and cnt == n and np.array_equal(got, offs)


# ------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _marshaler(spec, fast, dev):
    from xdrpp_amd import marshal as M
    return M.Marshaler(M.Plan(_cp(), {"specialize": spec, "index_fast": fast}), dev)


PLANS = [(spec, fast) for spec in (1, 0) for fast in (1, 2, 0)]

# Good streams the walk holds itself (its flag), generated parse, index_fast
# 1 and 2: (mode, kind) -> bands.  On an MI355X every one held (DESIGN.md
# 4.3.2 has the table, and what the windowed walk gave before its missed
# segments went to rxs_fix: two streams of 36).
HELD = {(mode, kind): set(BANDS) for mode in MODES for kind in KINDS}


def _same(mar, y, k, maxlen, want, dev, tag):
    w, wcnt, wrc, wer = want
    got, gcnt, err, tail = _gpu_index(mar, y, k, maxlen, dev, ws_tail=True)
    assert np.array_equal(got, w), tag
    assert gcnt == wcnt, tag
    assert (err.code if err else 0) == wrc, tag
    if err:
        assert err.record == wer, tag
    return tail


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", BANDS)
def test_gpu_index_bands(dev, B, kind):
    """Both modes, the generated and the interpreted parse, the walk gated by
    the host, asynchronous and off, good and damaged streams: the
    restatement's offsets, count, error and error record; and on the good
    streams of HELD the walk's own flag."""
    for mode in MODES:
        x, offs, n, maxlen = mode_stream(B, kind, mode)
        cases = damaged(x, offs, n, B) + damaged(x, offs, n, B + 1)[5:]
        wants = [O.index_records(_cp(), y, k, maxlen) for _, y, k in cases]
        for spec, fast in PLANS:
            mar = _marshaler(spec, fast, dev)
            for (label, y, k), want in zip(cases, wants):
                tail = _same(mar, y, k, maxlen, want, dev, (mode, spec, fast, label))
                if label == "good" and spec and fast:
                    held = _fast_flag(tail)
                    print(f"HOLD {mode} {kind} {B} fast={fast} flag={held}")
                    if B in HELD.get((mode, kind), ()):
                        assert held == 1, (mode, fast)


@pytest.mark.gpu
def test_gpu_index_past_window_record(dev):
    """One record 4 bytes past the window among short ones: INDEX_LONG at its
    index from the windowed index, the full index from the whole one."""
    x, offs, n, at = past_window_stream()
    for maxlen in (A.INDEX_MAX_MSG, A.MAX_MSG):
        want = O.index_records(_cp(), x, n, maxlen)
        assert want[2] == (A.ERR_INDEX_LONG if maxlen == A.INDEX_MAX_MSG else 0)
        for spec, fast in PLANS:
            _same(_marshaler(spec, fast, dev), x, n, maxlen, want, dev, (maxlen, spec, fast))


# ------------------------------------------------ the rxs_fix list's cap
FIX_CAP = 4096  # kRxsFixCap


def fix_stream(nrec):
    """nrec records of 14000-16000 bytes and nothing between them: each
    reaches over the whole segment after the one it starts in, so
    rxs_check<LONG> lists at least a segment per record."""
    rng = np.random.default_rng(5)
    unit = [rec(i, _rand(rng, 4 * int(rng.integers(3500 - 4, 4000 - 4))), b"") for i in range(43)]
    x, offs, n = _offsets(unit)
    x, offs, n = tiled(x, offs, n, -(-nrec // n))
    return x[:int(offs[nrec])], offs[:nrec + 1], nrec


def _fix_listed(tail):
    return int(tail[8:16].view(np.uint64)[0])  # rxs_fix's list count: flag[2..3]


FIX_CAP_WINDOW = 128  # kRxsFixCapWindow


@pytest.mark.gpu
@pytest.mark.parametrize("nrec,maxlen,cap,over", [
    (2400, A.MAX_MSG, FIX_CAP, False), (3000, A.MAX_MSG, FIX_CAP, True),
    (60, A.INDEX_MAX_MSG, FIX_CAP_WINDOW, False), (200, A.INDEX_MAX_MSG, FIX_CAP_WINDOW, True)],
    ids=["whole_under_cap", "whole_over_cap", "window_under_cap", "window_over_cap"])
def test_gpu_index_fix_cap(dev, nrec, maxlen, cap, over):
    """Both sides of rxs_fix's cap, in the walk over records of any length
    and in the one over records up to the window: under it the fix wave
    decides the listed segments and the walk holds the index; over it the
    call goes through the list ranking and is still exact.
    Observed on an MI355X: the list holds about 1.56 segments per record, not
    one -- the segment a record starts in (its exit passes over the next),
    and more often than not the one it ends in, whose look-back lies in the
    payload and whose guess then misses: 3900 records listed 6104 segments,
    4300 listed 6724.  So the record counts here, not 4000 and 4300."""
    import torch
    x, offs, n = fix_stream(nrec)
    sizes = np.diff(offs.astype(np.int64))
    assert 14000 <= sizes.min() and sizes.max() <= 16000
    want = O.index_records(_cp(), x, n, maxlen)
    assert want[2] == 0 and want[1] == n and np.array_equal(want[0], offs)
    mar = _marshaler(1, 1, dev)
    tail = _same(mar, x, n, maxlen, want, dev, nrec)
    # the call's time once more, stream and buffers on the device, and the
    # list ranking's beside it (not asserted)
    L = A.lib()
    dx = _dev(x, dev)
    ws = torch.empty(L.xdrg_index_workspace_size(x.size, maxlen), dtype=torch.uint8, device=dev)
    out = torch.empty(n + 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ms = []
    for m in (mar, _marshaler(1, 0, dev)):
        m.status.init(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        A.check(L.xdrg_index_records(m.plan.handle, dx.data_ptr(), x.size, n, maxlen, out.data_ptr(),
                                     cnt.data_ptr(), ws.data_ptr(), ws.numel(), m.status.ptr, s), "index")
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    listed, held = _fix_listed(tail), _fast_flag(tail)
    print(f"FIX nrec={nrec} maxlen={maxlen} bytes={x.size} listed={listed} flag={held} "
          f"call={ms[0]:.2f} ms index_fast=0: {ms[1]:.2f} ms")
    if over:
        assert listed > cap and held == 0
    else:
        assert 0 < listed <= cap and held == 1


# ------------------------- a captured stream with a record past the window
def capture_stream(long_enough):
    """Three short records, one of 20 KiB, three short ones (under WALK_MIN
    bytes); long_enough: then short ones until the walk runs."""
    rng = np.random.default_rng(9)
    short = lambda i: rec(i, _rand(rng, int(rng.integers(0, 200))), b"name")  # noqa: E731
    out = [short(i) for i in range(3)] + [rec(3, _rand(rng, 20 << 10), b"")] + [short(i) for i in range(4, 7)]
    while long_enough and sum(map(len, out)) < WALK_MIN + 1000:
        out.append(short(len(out)))
    return _offsets(out)


def test_oracle_capture_streams():
    for long_enough in (False, True):
        x, offs, n = capture_stream(long_enough)
        assert (x.size >= WALK_MIN) == long_enough
        got, cnt, rc, _ = O.index_records(_cp(), x, n, A.MAX_MSG)
        assert rc == 0 and cnt == n and np.array_equal(got, offs)
        got, cnt, rc, er = O.index_records(_cp(), x, n, A.INDEX_MAX_MSG)
        assert rc == A.ERR_INDEX_LONG and er == 3


def _captured_index(mar, x, n, dev):
    """xdrg_index_records(max_rec_len = XDRG_MAX_MSG) captured into a graph
    and replayed once: (offsets, count, error, flag)."""
    import torch
    from xdrpp_amd import marshal as M
    L = A.lib()
    dx = _dev(x, dev)
    ws = torch.empty(L.xdrg_index_workspace_size(x.size, A.MAX_MSG), dtype=torch.uint8, device=dev)
    out = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)

    def call(s, what):
        A.check(L.xdrg_index_records(mar.plan.handle, dx.data_ptr(), x.size, n, A.MAX_MSG, out.data_ptr(),
                                     cnt.data_ptr(), ws.data_ptr(), ws.numel(), mar.status.ptr, s), what)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm: plan tables and kernels uploaded outside the capture
        mar.status.init(side.cuda_stream)
        call(side.cuda_stream, "index (warm)")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.fill_(-1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(torch.cuda.current_stream().cuda_stream, "index (capture)")
    s = torch.cuda.current_stream().cuda_stream
    mar.status.init(s)
    g.replay()
    torch.cuda.synchronize()
    err = M.error_from(mar.plan, mar.status.read(s))
    w0 = L.xdrg_index_workspace_size(x.size, A.INDEX_MAX_MSG)
    return (out.cpu().numpy().view(np.uint64), int(cnt.cpu().numpy().view(np.uint64)[0]), err,
            _fast_flag(ws[w0 - 256:w0].cpu().numpy()))


@pytest.mark.gpu
def test_gpu_index_capture_short_stream_past_window(dev):
    """The contract of include/xdrgpu.h: under 4 segments (27776 bytes) the
    walk does not run, and on a stream being captured nothing else follows a
    record past the window -- the captured call reports INDEX_LONG at it, as
    the windowed index does, while the eager call indexes the stream."""
    x, offs, n = capture_stream(False)
    mar = _marshaler(1, 1, dev)
    want = O.index_records(_cp(), x, n, A.INDEX_MAX_MSG)
    got, cnt, err, flag = _captured_index(mar, x, n, dev)
    assert err is not None and err.code == A.ERR_INDEX_LONG == want[2] and err.record == want[3] == 3
    assert np.array_equal(got, want[0]) and cnt == want[1]
    assert flag == 0
    _same(mar, x, n, A.MAX_MSG, O.index_records(_cp(), x, n, A.MAX_MSG), dev, "eager")
    got, cnt, err = _gpu_index(mar, x, n, A.MAX_MSG, dev)
    assert err is None and cnt == n and np.array_equal(got, offs)


@pytest.mark.gpu
def test_gpu_index_capture_long_stream_past_window(dev):
    """From 27776 bytes on the captured walk over the whole stream runs and
    holds the same records."""
    x, offs, n = capture_stream(True)
    got, cnt, err, flag = _captured_index(_marshaler(1, 1, dev), x, n, dev)
    assert err is None and cnt == n and np.array_equal(got, offs)
    assert flag == 1


# ------------------------------------------------ record marks (mark_rx)
MSG_KINDS = ["random", "marks"]
MSG_MAX = [A.INDEX_MAX_MSG, 1 << 20]


@functools.lru_cache(maxsize=None)
def mark_stream(B, kind):
    """Record-marked messages: about one in three B - 4, B or B + 4 bytes
    with its mark, the rest short.  random: random bodies.  marks: every
    body word is a last-fragment mark of a small size, a multiple of 4 --
    chains of decoys."""
    rng = np.random.default_rng(2000 * B + MSG_KINDS.index(kind))
    out, size = [], 0
    while size < TOTAL:
        if rng.integers(0, 3) == 0:
            sz = B + 4 * int(rng.integers(-1, 2)) - 4
        else:
            sz = 4 * int(rng.integers(0, 60))
        if kind == "marks":
            body = (np.uint32(0x80000000) | (4 * rng.integers(0, 64, sz // 4)).astype(np.uint32)).astype(">u4").tobytes()
        else:
            body = _rand(rng, sz)
        out.append((0x80000000 | sz).to_bytes(4, "big") + body)
        size += 4 + sz
    return _offsets(out)


@pytest.mark.parametrize("kind", MSG_KINDS)
@pytest.mark.parametrize("B", BANDS)
def test_oracle_frames_the_mark_streams(B, kind):
    x, offs, n = mark_stream(B, kind)
    assert x.size >= TOTAL and {B - 4, B, B + 4} <= set(np.diff(offs.astype(np.int64)).tolist())
    for maxlen in MSG_MAX:
        rc, cnt, got = O.index_msgs(x, maxlen)
        assert rc == 0 and cnt == n and np.array_equal(got, offs), maxlen


@pytest.mark.gpu
@pytest.mark.parametrize("B", BANDS)
def test_gpu_index_msgs_bands(dev, B):
    """xdrg_index_msgs (the same walk through mark_rx) against the
    restatement's read_message framing, in one window and past it."""
    for kind in MSG_KINDS:
        x, offs, n = mark_stream(B, kind)
        for label, y, k in damaged(x, offs, n, B) + damaged(x, offs, n, B + 1)[5:]:
            for maxlen in MSG_MAX:
                want = O.index_msgs(y, maxlen, k)
                got = device_index(y, dev, maxlen, k)
                assert got[:2] == want[:2], (kind, label, maxlen)
                assert np.array_equal(got[2], want[2]), (kind, label, maxlen)
