"""xdrg_sort on the device (Marshaler.sort / unique / launch_sort): the
reference's recorded std::stable_sort and std::unique of every pool of
tests/golden/sort.json, then the sizes, input orders, frames, long lists and
bad references at which the kernels can go wrong.  Expected results come
from the recorded ranks (sort_fixture.expected_rows) or from how the values
are built; the property test checks the order with xdrg_compare."""
import struct
import sys

import numpy as np
import pytest

import sort_fixture as F
from test_gpu_compare import _chain, _recvar, _rp_list
from xdrpp_amd import _abi as A
from xdrpp_amd import objects as OBJ
from xdrpp_amd import schemas as S
from xdrpp_amd import workloads as W
from xdrpp_amd.xdr_types import compile_plan

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_MAR = {}


def _mar(t, dev):
    from xdrpp_amd import marshal as M
    if id(t) not in _MAR:
        _MAR[id(t)] = M.Marshaler(M.Plan(t), dev)
    return _MAR[id(t)]


def _dev(a, dev):
    if a is None or a.size == 0:
        return None
    return torch.from_numpy(np.array(a, copy=True)).to(dev)  # (the fixture's arrays are read-only)


def _sort(t, dev, nat, heap, n):
    """(perm, first, m, distinct) as numpy / int."""
    s = _mar(t, dev).sort(_dev(nat, dev), n, _dev(heap, dev))
    return s.perm.cpu().numpy().astype(np.int64), s.first.cpu().numpy(), s.sortable, s.distinct


def _check(got, want):
    perm, first, m, distinct = got
    wperm, wfirst, wm, wdistinct = want
    assert (m, distinct) == (wm, wdistinct)
    assert np.array_equal(perm, wperm), np.nonzero(perm != np.asarray(wperm))[0][:8]
    assert np.array_equal(first, wfirst), np.nonzero(first != np.asarray(wfirst))[0][:8]


@pytest.fixture(params=[True, False], ids=["tile", "global"])
def tile(request, monkeypatch):
    """The narrow passes in one LDS launch, or every pass in global memory."""
    if not request.param:
        monkeypatch.setenv("XDRG_SORT_TILE", "0")
    return request.param


# ------------------------------------------------------------- fixture pools
@pytest.mark.parametrize("name", list(F.TYPES))
def test_fixture_pools(dev, name, tile):
    p = F.pool(name)
    _check(_sort(F.TYPES[name], dev, p.nat, p.heap, p.n), (p.perm, p.first_all, p.m, p.distinct))


# ------------------------------------------------------- sizes and stability
def _rows(p, idx):
    return p.nat.reshape(p.n, p.cp.stride)[idx].reshape(-1)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 16, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("name", ["rec128", "recvar"])
def test_sizes_and_stability(dev, name, n, tile):
    """n rows drawn from 20 pool members (an unsortable one among them), so
    most values repeat: the order is the stable argsort of the recorded
    classes."""
    p = F.pool(name)
    rng = np.random.default_rng(1000 + n)
    members = np.concatenate([rng.permutation(p.sorted)[:19], p.unsortable[:1]])
    idx = members[rng.integers(0, len(members), n)]
    _check(_sort(F.TYPES[name], dev, _rows(p, idx), p.heap, n), F.expected_rows(p, idx))


# -------------------------------------------------------------- input orders
@pytest.mark.parametrize("name", ["rec128", "recvar"])
def test_input_orders(dev, name, tile):
    p = F.pool(name)
    n = 300
    rng = np.random.default_rng(7)
    t = F.TYPES[name]
    asc = p.sorted[np.sort(rng.integers(0, p.m, n))]
    want = F.expected_rows(p, asc)
    assert np.array_equal(want[0], np.arange(n))
    _check(_sort(t, dev, _rows(p, asc), p.heap, n), want)
    desc = asc[::-1].copy()
    want = F.expected_rows(p, desc)
    assert want[0][0] > want[0][-1]
    _check(_sort(t, dev, _rows(p, desc), p.heap, n), want)
    same = np.full(n, p.sorted[5])
    one = np.zeros(n, dtype=np.uint8)
    one[0] = 1
    _check(_sort(t, dev, _rows(p, same), p.heap, n), (np.arange(n), one, n, 1))
    bad = p.unsortable[np.arange(n) % len(p.unsortable)]
    _check(_sort(t, dev, _rows(p, bad), p.heap, n), (np.arange(n), np.ones(n, dtype=np.uint8), 0, 0))
    ends = p.sorted[rng.integers(0, p.m, n)]
    ends[0] = p.unsortable[0]
    ends[n - 1] = p.unsortable[-1]
    want = F.expected_rows(p, ends)
    assert want[2] == n - 2 and want[0][-2:].tolist() == [0, n - 1]
    _check(_sort(t, dev, _rows(p, ends), p.heap, n), want)


def test_empty_batch(dev):
    s = _mar(S.recvar, dev).sort(None, 0)
    assert s.perm.numel() == 0 and s.first.numel() == 0 and (s.sortable, s.distinct) == (0, 0)
    assert _mar(S.recvar, dev).unique(None, 0).numel() == 0


# -------------------------------------------------------------------- frames
def test_register_frames_and_deep(dev, tile):
    """XDRG_SUB_FRAMES + 1 levels: unsortable.  Exactly XDRG_SUB_FRAMES:
    sorted by the innermost element; the shallow value is greater than both
    (its second level holds b"x" where theirs hold b"m")."""
    K = A.SUB_FRAMES
    vals = [_chain(K, b"y"), _chain(K + 1, b"x"), _chain(K, b"x"), _chain(2, b"x"), _chain(K, b"x")]
    nat, heap = OBJ.stage(S.test_recursive, vals)
    _check(_sort(S.test_recursive, dev, nat, heap, len(vals)), ([2, 4, 0, 3, 1], [1, 0, 1, 1, 1], 4, 3))


def test_long_lists(dev, tile):
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    full, other = _rp_list(600), _rp_list(600, b"rooT")  # the last of 600 nodes decides ('T' < 't')
    nat, heap = OBJ.stage(S.rp__list, [full, other, full])
    _check(_sort(S.rp__list, dev, nat, heap, 3), ([1, 0, 2], [1, 1, 0], 3, 2))


# ------------------------------------------------------------ bad references
def test_bad_reference_is_unsortable(dev, tile):
    """A reference one byte past the heap length passed is read through by
    nobody; the tensor is 4 KiB longer than that length, so nothing leaves
    the allocation either way."""
    base = bytes(range(64))
    nat, heap = _recvar([(base, 0, b"c"), (base, 0, b"b"), (base, 0, b"a"), (base, 0, b"b")])
    st, off = compile_plan(S.recvar).stride, S.recvar.offsets["blob"]
    _, ln, _ = struct.unpack_from("<QII", nat, st + off)
    nat = nat.copy()
    struct.pack_into("<QII", nat, st + off, heap.size + 1 - ln, ln, 0)  # off + len = heap_len + 1
    big = torch.zeros(heap.size + 4096, dtype=torch.uint8, device=dev)
    big[:heap.size] = _dev(heap, dev)
    s = _mar(S.recvar, dev).sort(_dev(nat, dev), 4, big[:heap.size])
    _check((s.perm.cpu().numpy().astype(np.int64), s.first.cpu().numpy(), s.sortable, s.distinct),
           ([2, 3, 0, 1], [1, 1, 1, 1], 3, 3))


# --------------------------------------------------------------------- graph
def test_graph_capture_replays(dev):
    """A var plan with element subroutines, captured and replayed twice with
    the outputs refilled in between (the kernels keep no private memory:
    tests/test_sort_abi.py)."""
    p = F.pool("containertest")
    mar = _mar(S.containertest, dev)
    recs, heap = _dev(p.nat, dev), _dev(p.heap, dev)
    perm = torch.full((p.n,), -1, dtype=torch.int32, device=dev)
    first = torch.full((p.n,), 99, dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    ws = mar.sort_workspace(p.n)

    def check():
        assert np.array_equal(perm.cpu().numpy(), p.perm)
        assert np.array_equal(first.cpu().numpy(), p.first_all)
        assert counts.cpu().tolist() == [p.m, p.distinct]

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the plan's tables go up outside the capture
        mar.launch_sort(recs, p.n, perm, first, counts, heap, ws, stream=side.cuda_stream)
    torch.cuda.synchronize()
    check()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mar.launch_sort(recs, p.n, perm, first, counts, heap, ws, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        perm.fill_(-1)
        first.fill_(99)
        counts.fill_(-1)
        ws.fill_(0xee)
        g.replay()
        torch.cuda.synchronize()
        check()


# ------------------------------------------------------------------ property
@pytest.mark.parametrize("name", ["recvar", "containertest"])
def test_order_property(dev, name, tile):
    """4096 generated records, every fourth one of the second half a copy of
    an earlier one: perm is a permutation whose sortable part ascends under
    xdrg_compare, equivalent neighbours in input order, first = "the left
    neighbour is less", the unsortable records behind in input order."""
    n = 4096
    t = S.ALL[name]
    mar = _mar(t, dev)
    nat, heap = W.GENERATORS[name](n)
    st = mar.plan.stride
    rows = nat.reshape(n, st)
    rows[n // 2::4] = rows[:n // 2:4]
    recs, dheap = _dev(rows.reshape(-1), dev), _dev(heap, dev)
    s = mar.sort(recs, n, dheap)
    perm = s.perm.cpu().numpy().astype(np.int64)
    first = s.first.cpu().numpy()
    m = s.sortable
    assert np.array_equal(np.sort(perm), np.arange(n))
    own = mar.compare(recs, recs, n, dheap, dheap).cpu().numpy()
    assert m == int((own == A.CMP_EQUAL).sum()) and n - 64 <= m
    assert np.array_equal(perm[m:], np.nonzero(own != A.CMP_EQUAL)[0])
    g = recs.view(n, st)[s.perm.long()]
    nb = mar.compare(g[:-1].reshape(-1), g[1:].reshape(-1), n - 1, dheap, dheap).cpu().numpy()[:m - 1]
    assert np.isin(nb, [A.CMP_LESS, A.CMP_EQUAL]).all()
    eq = np.nonzero(nb == A.CMP_EQUAL)[0]
    assert eq.size >= n // 8 - 64 and (perm[eq] < perm[eq + 1]).all()
    assert first[0] == 1 and np.array_equal(first[1:m], nb == A.CMP_LESS) and first[m:].all()
    assert s.distinct == int(first[:m].sum())


# -------------------------------------------------------------------- unique
@pytest.mark.parametrize("name", ["recvar", "ContainsEnum"])
def test_unique(dev, name):
    p = F.pool(name)
    got = _mar(F.TYPES[name], dev).unique(_dev(p.nat, dev), p.n, _dev(p.heap, dev)).cpu().numpy()
    assert p.distinct < p.m
    assert np.array_equal(got, p.sorted[p.first == 1])
