"""GPU: per-record decode verdicts (xdrg_verify, include/xdrgpu.h "Per-record
decode verdicts"): the decode walk without stores, one verdict per record.

A verdict is what xdrg_decode reports for the record decoded alone, which is
what the restatement oracle returns for the slice (verdict_model.py):
decode_arg's view of a call (xdrpp/server.h:205-214), where one bad record
does not hide the others.  Real-reference anchors: the kbounded exceptions of
tests/golden/kat.json and the chains of tests/golden/deep.json."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, SMALL_N, golden

from xdrpp_amd import _abi as A
from xdrpp_amd import schemas as S
from xdrpp_amd.xdr_types import compile_plan
import verdict_model as V

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N = 512
SEVEN = list(SMALL_N)
FUZZED = SEVEN + ["numerics_validated"]


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def schema_type(name):
    return S.ALL.get(name) or S.CONTAINERS.get(name) or getattr(S, name)


def stream_of(name):
    """(xdr, offsets uint64 [n + 1]) of a schema's golden stream; fixed
    schemas' offsets are implied by their record size."""
    g = "numerics" if name == "numerics_validated" else name
    n = SMALL_N[g]
    xdr = golden(g, n, "xdr")
    fs = compile_plan(schema_type(name)).fixed_size
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(fs) if fs else golden(g, n, "offsets", np.uint64)
    assert offs.size == n + 1 and int(offs[-1]) == xdr.size
    return xdr, offs


def marshaler(name, dev):
    from xdrpp_amd import marshal as M
    return M.Marshaler(M.Plan(schema_type(name)), dev)


def span_verdicts(mar, dx, spans, stack_limit=A.DEFAULT_STACK_LIMIT):
    """verify() over explicit begin / end arrays at stride 16: (uint32 verdicts, bad_count)."""
    be = _dev(np.ascontiguousarray(spans, dtype=np.int64).reshape(-1, 2), mar.device)
    v, bad = mar.verify(dx, begin=be[:, 0], end=be[:, 1], stack_limit=stack_limit)
    return v.cpu().numpy().view(np.uint32), bad


@pytest.mark.parametrize("name", SEVEN)
def test_goldens_decode(dev, name):
    """The first 512 records of every golden stream: all verdicts 0."""
    mar = marshaler(name, dev)
    xdr, offs = stream_of(name)
    if mar.plan.is_fixed:  # implied offsets
        v, bad = mar.verify(_dev(xdr[:N * mar.plan.fixed_size], dev))
    else:
        v, bad = mar.verify(_dev(xdr, dev), _dev(offs[:N + 1].astype(np.int64), dev))
    assert v.numel() == N and v.dtype == torch.int32
    assert not v.cpu().numpy().any() and bad == 0


def test_reference_kats_in_one_batch(dev, kat):
    """The real reference's exceptions for the five kbounded inputs, as five
    spans of one batch: every record gets its own; xdrg_decode of the same
    batch reports record 1 alone."""
    from test_kat import kbounded
    from xdrpp_amd import marshal as M
    names = ["kbounded_in", "kbounded_over_blob", "kbounded_over_s", "kbounded_over_v", "kbounded_over_all"]
    parts = [np.frombuffer(bytes.fromhex(kat["errors"][k]["input"]), dtype=np.uint8) for k in names]
    x = np.concatenate(parts)
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    plan = M.Plan(kbounded, {"specialize": 0})  # (no kernels to generate for five records)
    mar = M.Marshaler(plan, dev)
    dx, doffs = _dev(x, dev), _dev(offs, dev)
    v, bad = mar.verify(dx, doffs)
    v = v.cpu().numpy().view(np.uint32)
    assert list(v & 0xFF) == [0, 3, 4, 3, 3] and bad == 4
    want = V.oracle_verdicts(plan.cp, x, np.stack([offs[:-1], offs[1:]], axis=1))
    assert np.array_equal(v, want)
    for r, k in enumerate(names):  # the reference's exception class and what()
        e = M.verdict_error(plan, v[r], r)
        if kat["errors"][k]["exception"] == "none":
            assert e is None
        else:
            assert isinstance(e, M.XdrOverflow) and e.what == kat["errors"][k]["what"] and e.record == r
    with pytest.raises(M.XdrRuntimeError) as ei:
        mar.decode(dx, 5, doffs)
    assert ei.value.record == 1 and ei.value.code == 3


def test_one_bad_record_does_not_hide_others(dev):
    """recvar_1024 with the name length of records 3, 500 and 1023 forged."""
    mar = marshaler("recvar", dev)
    xdr, offs = stream_of("recvar")
    x = xdr.copy()
    hit = [3, 500, 1023]
    for r in hit:
        a = int(offs[r])
        blob = int.from_bytes(x[a + 12:a + 16].tobytes(), "big")
        V.put_be(x, a + 16 + ((blob + 3) & ~3), 0xFFFFFFFF)  # string name<64>'s length word
    v, bad = mar.verify(_dev(x, dev), _dev(offs.astype(np.int64), dev))
    v = v.cpu().numpy().view(np.uint32)
    assert list(np.nonzero(v)[0]) == hit and bad == 3
    for r in hit:
        assert v[r] == V.oracle_verdict(mar.plan.cp, x, offs[r], offs[r + 1]) != 0


@pytest.mark.parametrize("name", FUZZED)
def test_fuzz_matches_oracle(dev, name):
    """512 records, a third with a word replaced, a third with their end
    moved, at explicit begin / end arrays 16 bytes apart: every verdict and
    the count are the oracle's for the slice, at the default stack limit and
    at 2.  The batch is a test only when the oracle itself calls at least a
    quarter of it bad and a quarter good.  At limit 2 a plan whose ops reach
    depth 3 must raise xdr_stack_overflow somewhere (plans that stay within
    depth 2 cannot)."""
    mar = marshaler(name, dev)
    cp = mar.plan.cp
    xdr, offs = stream_of(name)
    x, spans = V.fuzz_batch(xdr, offs, N, np.random.default_rng(7))
    dx = _dev(x, dev)
    want = V.oracle_verdicts(cp, x, spans)
    share = np.count_nonzero(want) / N
    assert 0.25 <= share <= 0.75, f"oracle bad share {share}"
    got, bad = span_verdicts(mar, dx, spans)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert bad == np.count_nonzero(want)
    want2 = V.oracle_verdicts(cp, x, spans, 2)
    got2, bad2 = span_verdicts(mar, dx, spans, 2)
    assert np.array_equal(got2, want2), np.nonzero(got2 != want2)[0][:8]
    assert bad2 == np.count_nonzero(want2)
    if mar.plan.max_depth > 2:
        assert np.any((got2 & 0xFF) == A.ERR_STACK_GET)


@pytest.fixture(scope="module")
def deep():
    with open(os.path.join(GOLD, "deep.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["rp__list", "test_recursive"])
def test_deep_records(dev, deep, name):
    """The real reference's chains: verdict 0 at get_limit and the oracle's
    xdr_stack_overflow one below.  rp__list's link is a tail container: no
    frame, any length.  test_recursive's `next` is not its last field: one
    frame a node, exact up to depth 16, past it exact or XDRG_ERR_INDEX_LONG
    (not decided)."""
    mar = marshaler(name, dev)
    cp = mar.plan.cp
    for e in deep[name]:
        x = np.frombuffer(bytes.fromhex(e["xdr"]), dtype=np.uint8).copy()
        lim, depth = int(e["get_limit"]), int(e["depth"])
        dx = _dev(x, dev)
        for sl in (lim, lim - 1):
            want = V.oracle_verdict(cp, x, 0, x.size, sl)
            assert (want == 0) == (sl == lim) and (sl == lim or want & 0xFF == A.ERR_STACK_GET)
            got, bad = span_verdicts(mar, dx, [[0, x.size]], sl)
            if name == "rp__list" or depth <= A.INDEX_FRAMES:
                assert got[0] == want, (depth, sl, hex(got[0]), hex(want))
            else:
                assert got[0] == want or got[0] & 0xFF == A.ERR_INDEX_LONG, (depth, sl, hex(got[0]))
            assert bad == (got[0] != 0)


@pytest.mark.parametrize("n", [1, 65])
def test_bogus_spans(dev, n):
    """Spans a forged index could hold -- end < begin, end > len, a misaligned
    begin, an empty span for a plan that needs bytes -- beside good records:
    the verdicts the header defines, nothing outside the stream read."""
    mar = marshaler("recvar", dev)
    xdr, offs = stream_of("recvar")
    L = xdr.size
    a1, b1 = int(offs[1]), int(offs[2])
    bogus = [(b1, a1), (a1, L + 4), (L + 4, L + 8), (1 << 62, (1 << 62) + 64), (a1 + 2, b1 + 2),
             (a1 + 1, b1), (a1, a1), (L, L), (a1, b1 - 1)]
    want_bogus = [1, 1, 1, 1, 1, 1, V.verdict(0, A.ERR_OVERFLOW_GET), V.verdict(0, A.ERR_OVERFLOW_GET),
                  V.verdict(V.RECORD_LEVEL, A.ERR_SIZE_NOT_MULT4)]
    dx = _dev(xdr, dev)
    if n == 1:
        for span, want in zip(bogus, want_bogus):
            assert V.oracle_verdict(mar.plan.cp, xdr, *span) == want
            got, bad = span_verdicts(mar, dx, [span])
            assert got[0] == want and bad == 1, (span, hex(got[0]))
        got, bad = span_verdicts(mar, dx, [(a1, b1)])
        assert got[0] == 0 and bad == 0
        return
    spans = [bogus[(r // 2) % len(bogus)] if r % 2 else (int(offs[r]), int(offs[r + 1])) for r in range(n)]
    want = V.oracle_verdicts(mar.plan.cp, xdr, np.array(spans, dtype=np.int64))
    assert np.count_nonzero(want) == n // 2
    got, bad = span_verdicts(mar, dx, spans)
    assert np.array_equal(got, want) and bad == n // 2


def test_graph_capture_replays_follow_the_data(dev):
    """xdrg_verify captured once and replayed over a stream that changes
    between replays: verdicts and the count follow the data, so the count is
    zeroed again by every replay."""
    mar = marshaler("recvar", dev)
    cp = mar.plan.cp
    xdr, offs = stream_of("recvar")
    n = 300
    spans = np.stack([offs[:n], offs[1:n + 1]], axis=1).astype(np.int64)
    dx = _dev(xdr, dev)
    doffs = _dev(offs[:n + 1].astype(np.int64), dev)
    verdicts = torch.zeros(n, dtype=torch.int32, device=dev)
    bad = torch.full((1,), 77, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm: the plan's tables outside the capture
        mar.launch_verify(dx, doffs.data_ptr(), doffs.data_ptr() + 8, 8, n, verdicts, bad, stream=side.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mar.launch_verify(dx, doffs.data_ptr(), doffs.data_ptr() + 8, 8, n, verdicts, bad,
                          stream=torch.cuda.current_stream().cuda_stream)
    x = xdr.copy()
    for damaged in ([], [5, 64, 299], [5, 64, 299], [7], []):
        x[:] = xdr
        for r in damaged:
            V.put_be(x, int(offs[r]) + 12, 0xFFFFFFFF)  # opaque blob<256>'s length word
        dx.copy_(_dev(x, dev))
        verdicts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = V.oracle_verdicts(cp, x, spans)
        assert list(np.nonzero(want)[0]) == damaged
        assert np.array_equal(verdicts.cpu().numpy().view(np.uint32), want)
        assert int(bad.item()) == len(damaged)
