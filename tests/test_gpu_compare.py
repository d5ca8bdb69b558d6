"""xdrg_compare on the device (Marshaler.compare / equal): the reference's
recorded operator<=> and operator== on every pair of tests/golden/
compare.json, then the shapes, word kinds, byte alignments, containers,
frames and bad references at which the two kernels can go wrong.  Expected
results of the hand-built pairs follow from how they are built; the Python
model (tests/compare_model.py, pinned to the reference by
tests/test_compare_model.py) is asserted beside them."""
import struct
import sys

import numpy as np
import pytest

import compare_fixture as F
import compare_model as CM
from xdrpp_amd import _abi as A
from xdrpp_amd import objects as OBJ
from xdrpp_amd import schemas as S
from xdrpp_amd import workloads as W
from xdrpp_amd.xdr_types import Bool, Double, Hyper, Int, OpaqueArray, Struct, compile_plan

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LESS, EQUAL, GREATER, UNORDERED, DEEP, BADREF = CM.LESS, CM.EQUAL, CM.GREATER, CM.UNORDERED, CM.DEEP, CM.BADREF


def _dev(a, dev):
    if a is None or a.size == 0:
        return None
    return torch.from_numpy(np.array(a, copy=True)).to(dev)  # (the fixture's arrays are read-only)


_MAR = {}


def _mar(t, dev):
    from xdrpp_amd import marshal as M
    if id(t) not in _MAR:
        _MAR[id(t)] = M.Marshaler(M.Plan(t), dev)
    return _MAR[id(t)]


def _compare(t, dev, nat_a, heap_a, nat_b, heap_b, n, model=True):
    """The device's results (int8[n]); equal() must be their == 0, and the
    model must give the same."""
    mar = _mar(t, dev)
    da, db, ha, hb = _dev(nat_a, dev), _dev(nat_b, dev), _dev(heap_a, dev), _dev(heap_b, dev)
    got = mar.compare(da, db, n, ha, hb).cpu().numpy()
    eq = mar.equal(da, db, n, ha, hb).cpu().numpy()
    assert np.array_equal(eq, got == EQUAL)
    if model:
        want = CM.compare(mar.plan.cp, nat_a, heap_a, nat_b, heap_b, n)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    return got


# ------------------------------------------------------------ fixture pairs
@pytest.mark.parametrize("name", list(F.TYPES))
def test_fixture_pairs(dev, name):
    b = F.batch(name)
    got = _compare(F.TYPES[name], dev, b.nat_a, b.heap_a, b.nat_b, b.heap_b, b.n, model=False)
    bad = np.nonzero(got != b.cmp)[0]
    assert bad.size == 0, [(int(i), b.how[i], int(got[i]), int(b.cmp[i])) for i in bad[:8]]
    mar = _mar(F.TYPES[name], dev)
    eq = mar.equal(_dev(b.nat_a, dev), _dev(b.nat_b, dev), b.n, _dev(b.heap_a, dev), _dev(b.heap_b, dev))
    assert np.array_equal(eq.cpu().numpy(), b.eq)


# ------------------------------------------------------------- batch shapes
def _pick(b, want):
    return int(np.nonzero(b.cmp == want)[0][0])


@pytest.mark.parametrize("name", ["rec128", "recvar"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_shapes(dev, name, n):
    """Fixture pairs repeated: an equal pair everywhere, a deciding pair at
    the first and at the last index (wave and grid tails)."""
    b = F.batch(name)
    idx = np.full(n, _pick(b, 0))
    idx[n - 1] = _pick(b, 1)
    idx[0] = _pick(b, -1)
    st = b.cp.stride
    rows_a = b.nat_a.reshape(b.n, st)[idx].reshape(-1)
    rows_b = b.nat_b.reshape(b.n, st)[idx].reshape(-1)
    got = _compare(F.TYPES[name], dev, rows_a, b.heap_a, rows_b, b.heap_b, n)
    assert np.array_equal(got, b.cmp[idx])
    assert got[0] == LESS and (n == 1 or (got[-1] == GREATER and not got[1:-1].any()))


# -------------------------------------------------------- fixed chunk kernel
R128 = np.dtype([(f"a{i}", "<i4") for i in range(8)] + [(f"u{i}", "<u8") for i in range(6)]
                + [(f"d{i}", "<f8") for i in range(6)])
assert R128.itemsize == 128
R128_FIELDS = list(R128.names)


def _r128_base(n):
    r = np.zeros(n, dtype=R128)
    for k, f in enumerate(R128_FIELDS):
        r[f] = 10 + k
    return r


def _as_u8(r):
    return r.view(np.uint8).reshape(-1).copy()


def test_rec128_each_field_decides(dev):
    a = _r128_base(40)
    b = a.copy()
    for k, f in enumerate(R128_FIELDS):
        b[f][k] += 1          # pair k: b's field k is larger -> less
        a[f][20 + k] += 1     # pair 20 + k: the other way round -> greater
    got = _compare(S.rec128, dev, _as_u8(a), None, _as_u8(b), None, 40)
    assert np.array_equal(got, [LESS] * 20 + [GREATER] * 20)


def test_rec128_lower_field_wins(dev):
    pairs = [(0, 1), (0, 3), (3, 4), (1, 19), (7, 8), (8, 9), (9, 10), (13, 14), (14, 19), (18, 19), (2, 12), (11, 16)]
    a = _r128_base(len(pairs))
    b = a.copy()
    for p, (lo, hi) in enumerate(pairs):  # fields in one chunk, neighbouring chunks, first and last chunk
        b[R128_FIELDS[lo]][p] -= 1        # the lower field says greater
        b[R128_FIELDS[hi]][p] += 1        # a later one says less
    got = _compare(S.rec128, dev, _as_u8(a), None, _as_u8(b), None, len(pairs))
    assert np.array_equal(got, [GREATER] * len(pairs))


def test_rec128_unsigned_hyper_and_nan(dev):
    a = _r128_base(4)
    b = a.copy()
    a["u2"][0] = 0xFFFFFFFFFFFFFFFF  # unsigned: greater than 1
    b["u2"][0] = 1
    a["a5"][1] = -1                  # signed: less than 1
    b["a5"][1] = 1
    a["d4"][2] = b["d4"][2] = np.nan  # identical bytes, unordered
    a["d0"][3] = -0.0                 # different bytes, equivalent
    b["d0"][3] = 0.0
    got = _compare(S.rec128, dev, _as_u8(a), None, _as_u8(b), None, 4)
    assert np.array_equal(got, [GREATER, LESS, UNORDERED, EQUAL])


# hyper, double, a bool and an opaque[3] with native padding around them: stride 32
FX = Struct("fx", [("h", Hyper), ("d", Double), ("b", Bool), ("i", Int), ("o", OpaqueArray(3))])
FXD = np.dtype({"names": ["h", "d", "b", "i", "o"], "formats": ["<i8", "<f8", "u1", "<i4", ("u1", 3)],
                "offsets": [0, 8, 16, 20, 24], "itemsize": 32})


def test_fixed_plan_halves_signs_and_padding(dev):
    assert compile_plan(FX).stride == 32
    cases = [  # (field, a, b, result)
        ("h", 0x0000000100000005, 0x0000000200000005, LESS),     # the high word only
        ("h", 0x0000000100000006, 0x0000000100000005, GREATER),  # the low word only
        ("h", -1, 1, LESS),                                       # negative against positive
        ("h", 1, -(2 ** 63), GREATER),
        ("d", 1.0, 2.0, LESS),                                    # high word only
        ("d", 1.0, 1.0000000000000002, LESS),                     # low word only
        ("d", -1.0, -2.0, GREATER),                               # (bit patterns order the other way)
        ("d", -0.0, 0.0, EQUAL),
        ("d", float("nan"), float("nan"), UNORDERED),
        ("d", float("nan"), 1.0, UNORDERED),
        ("b", 2, 1, EQUAL),                                       # any nonzero byte is true
        ("b", 0, 2, LESS),
        ("b", 0x80, 0, GREATER),
        ("i", -5, 3, LESS),
        ("o", (1, 2, 0x7f), (1, 2, 0x80), LESS),                  # unsigned chars
        ("o", (9, 0, 0), (1, 200, 200), GREATER),                 # the first byte decides
    ]
    n = len(cases) + 2
    rng = np.random.default_rng(5)
    raw_a = rng.integers(0, 256, n * 32, dtype=np.uint8)  # garbage in the padding, differing
    raw_b = rng.integers(0, 256, n * 32, dtype=np.uint8)
    a, b = raw_a.view(FXD), raw_b.view(FXD)  # (views: a copy of a padded dtype need not keep the padding)
    for f in FXD.names:
        a[f] = 7
        b[f] = 7
    want = []
    for k, (f, va, vb, res) in enumerate(cases):
        a[f][k] = va
        b[f][k] = vb
        want.append(res)
    # NaN behind an earlier differing field; the last pair differs in padding only
    a["h"][n - 2], a["d"][n - 2] = 6, np.nan
    want += [LESS, EQUAL]
    assert not np.array_equal(raw_a[-32:], raw_b[-32:])
    got = _compare(FX, dev, raw_a, None, raw_b, None, n)
    assert np.array_equal(got, want)


def test_numerics_takes_the_walk(dev):
    cp = compile_plan(S.numerics)
    assert cp.stride == 56 and cp.stride % 16  # not the chunk kernel's
    b = F.batch("numerics")
    rng = np.random.default_rng(9)
    na, nb = b.nat_a.copy().reshape(b.n, 56), b.nat_b.copy().reshape(b.n, 56)
    off = S.numerics.offsets
    pad = [i for i in range(56) if not any(off[f] <= i < off[f] + t.size for f, t in S.numerics.fields)]
    assert pad
    na[:, pad] = rng.integers(0, 256, (b.n, len(pad)), dtype=np.uint8)
    nb[:, pad] = rng.integers(0, 256, (b.n, len(pad)), dtype=np.uint8)
    got = _compare(S.numerics, dev, na.reshape(-1), None, nb.reshape(-1), None, b.n)
    assert np.array_equal(got, b.cmp)


# --------------------------------------------------------------------- bytes
def _recvar(recs):
    """recvar records with their blobs where the test wants them: rec =
    (blob, misalignment 0..15, name); each blob in a 16-aligned slot of its
    own, `mis` bytes in."""
    st = compile_plan(S.recvar).stride
    off = S.recvar.offsets
    nat = bytearray(st * len(recs))
    heap = bytearray()
    for i, (blob, mis, name) in enumerate(recs):
        heap.extend(bytes(-len(heap) % 16))
        heap.extend(b"\xee" * mis)
        bo = len(heap)
        heap.extend(blob)
        no = len(heap)
        heap.extend(name)
        struct.pack_into("<Qi", nat, i * st + off["id"], 77, -3)
        struct.pack_into("<QII", nat, i * st + off["blob"], bo, len(blob), 0)
        struct.pack_into("<QII", nat, i * st + off["name"], no, len(name), 0)
        struct.pack_into("<d", nat, i * st + off["score"], 0.5)
    heap.extend(bytes(-len(heap) % 4))
    return np.frombuffer(bytes(nat), dtype=np.uint8).copy(), np.frombuffer(bytes(heap), dtype=np.uint8).copy()


def test_blob_differs_at_byte_k_at_every_alignment(dev):
    base = bytes((37 * j + 11) % 200 + 16 for j in range(256))
    ra, rb, want = [], [], []
    ks = [(k, k % 16, (7 * k + 3) % 16) for k in list(range(32)) + [255]]
    ks += [((17 * i + 5 * j) % 256, i, j) for i in range(16) for j in range(16)]  # offsets 0..15, independently
    for k, ma, mb in ks:
        other = bytearray(base)
        other[k] += 1
        ra.append((base, ma, b"nm"))
        rb.append((bytes(other), mb, b"nm"))
        want.append(LESS)
    hi = bytearray(base)
    hi[100] = 0x7f
    lo = bytearray(base)
    lo[100] = 0x80
    ra.append((bytes(hi), 3, b"nm"))   # 0x7f against 0x80: unsigned chars
    rb.append((bytes(lo), 9, b"nm"))
    want.append(LESS)
    for la, lb, res in [(0, 1, LESS), (1, 0, GREATER), (255, 256, LESS), (256, 255, GREATER), (0, 0, EQUAL),
                        (256, 256, EQUAL), (19, 19, EQUAL)]:
        ra.append((base[:la], 5, b"nm"))  # an equal prefix: the lengths decide
        rb.append((base[:lb], 12, b"nm"))
        want.append(res)
    ra.append((b"", 1, b"abc"))  # 0 against 0 at different offsets, then the name decides
    rb.append((b"", 14, b"abd"))
    want.append(LESS)
    na, ha = _recvar(ra)
    nb, hb = _recvar(rb)
    got = _compare(S.recvar, dev, na, ha, nb, hb, len(want))
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- containers
def _ct(uvec, s0=b"hello", s1=b"world"):
    return {"uvec": uvec, "sarr": [s0, s1]}


def test_containers(dev):
    f4 = lambda i: (4, {"i": i})  # noqa: E731
    f12 = lambda i, d: (12, {"i": i, "d": d})  # noqa: E731
    three = [f4(1), f12(2, 0.5), f4(3)]
    cases = [
        (_ct([]), _ct([]), EQUAL),
        (_ct([]), _ct(three), LESS),
        (_ct(three), _ct([]), GREATER),
        (_ct(three), _ct(three), EQUAL),
        (_ct(three), _ct([f4(1), f12(2, 0.5), f4(4)]), LESS),          # the last element
        (_ct([f4(1), f12(2, 0.75), f4(3)]), _ct(three), GREATER),
        (_ct(three), _ct(three + [f4(-9)]), LESS),                      # 3 against 4, equal prefix
        (_ct(three + [f4(-9)]), _ct(three), GREATER),
        (_ct([f4(1)]), _ct([f12(1, 0.0)]), LESS),                       # the discriminant only
        (_ct([f12(0, float("nan"))]), _ct([f12(0, float("nan"))]), UNORDERED),
        (_ct(three, b"hello"), _ct(three, b"hellp"), LESS),             # behind the container
        (_ct([f4(2)], b"a"), _ct([f4(1), f4(5)], b"b"), GREATER),       # an element before the counts
    ]
    na, ha = OBJ.stage(S.containertest, [c[0] for c in cases])
    nb, hb = OBJ.stage(S.containertest, [c[1] for c in cases])
    got = _compare(S.containertest, dev, na, ha, nb, hb, len(cases))
    assert np.array_equal(got, [c[2] for c in cases])


# -------------------------------------------------------------------- frames
def _chain(depth, inner, mid=b"m", level1=b"m"):
    """test_recursive nested `depth` levels through nextvec, each level's
    container two elements long with the chain in the first (so no level is
    in tail position and each takes a frame)."""
    leaf = {"elem": b"leaf", "next": None, "nextvec": []}
    node = {"elem": inner, "next": None, "nextvec": []}
    for lvl in range(depth - 1, 0, -1):
        node = {"elem": level1 if lvl == 1 else mid, "next": None, "nextvec": [node, leaf]}
    return {"elem": b"top", "next": None, "nextvec": [node, leaf]}


def test_register_frames_and_deep(dev):
    K = A.SUB_FRAMES
    cases = [
        (_chain(K, b"x"), _chain(K, b"y"), LESS),           # exactly K frames, the innermost elem decides
        (_chain(K, b"x"), _chain(K, b"x"), EQUAL),
        (_chain(K + 1, b"x"), _chain(K + 1, b"y"), DEEP),   # one more: not compared
        (_chain(K + 1, b"x", level1=b"n"), _chain(K + 1, b"y"), GREATER),  # ... unless decided above
        (_chain(K + 1, b"x"), _chain(K + 1, b"x"), DEEP),
        (_chain(2, b"x"), _chain(2, b"x"), EQUAL),          # a deep neighbour leaves the others alone
    ]
    na, ha = OBJ.stage(S.test_recursive, [c[0] for c in cases])
    nb, hb = OBJ.stage(S.test_recursive, [c[1] for c in cases])
    got = _compare(S.test_recursive, dev, na, ha, nb, hb, len(cases))
    assert np.array_equal(got, [c[2] for c in cases])


def _rp_list(k, last_owner=b"root"):
    node = None
    for i in range(k - 1, -1, -1):
        node = {"rpcb_map": {"r_prog": 100000 + i, "r_vers": i % 5, "r_netid": b"tcp", "r_addr": b"0.0.0.0.0.%d" % i,
                             "r_owner": last_owner if i == k - 1 else b"root"}, "rpcb_next": node}
    return node


def test_linked_list_compares_in_one_frame(dev):
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    full, other, prefix = _rp_list(600), _rp_list(600, b"rooT"), _rp_list(599)
    cases = [(full, other, GREATER),   # the last of 600 nodes decides ('t' > 'T')
             (other, full, LESS),
             (full, full, EQUAL),
             (prefix, full, LESS),     # an absent pointer is less than a present one
             (full, prefix, GREATER)]
    na, ha = OBJ.stage(S.rp__list, [c[0] for c in cases])
    nb, hb = OBJ.stage(S.rp__list, [c[1] for c in cases])
    got = _compare(S.rp__list, dev, na, ha, nb, hb, len(cases))
    assert np.array_equal(got, [c[2] for c in cases])


# ------------------------------------------------------------ bad references
def test_bad_references(dev):
    """A reference one byte past the heap length passed is refused and read
    through by nobody; the tensors are 4 KiB longer than that length, so
    nothing leaves the allocation either way."""
    base = bytes(range(64))
    recs = [(base, 0, b"a"), (base, 0, b"b"), (base, 0, b"c")]
    na, ha = _recvar(recs)
    nb, hb = _recvar(recs)
    st, off = compile_plan(S.recvar).stride, S.recvar.offsets["blob"]
    bo, ln, _ = struct.unpack_from("<QII", na, st + off)
    na = na.copy()
    struct.pack_into("<QII", na, st + off, ha.size + 1 - ln, ln, 0)  # off + len = heap_len + 1
    mar = _mar(S.recvar, dev)
    big_a = torch.zeros(ha.size + 4096, dtype=torch.uint8, device=dev)
    big_b = torch.zeros(hb.size + 4096, dtype=torch.uint8, device=dev)
    big_a[:ha.size] = _dev(ha, dev)
    big_b[:hb.size] = _dev(hb, dev)
    got = mar.compare(_dev(na, dev), _dev(nb, dev), 3, big_a[:ha.size], big_b[:hb.size]).cpu().numpy()
    assert np.array_equal(got, [EQUAL, BADREF, EQUAL])
    assert np.array_equal(CM.compare(mar.plan.cp, na, ha, nb, hb, 3), got)
    # the same reference on b's side, and an element reference
    got = mar.compare(_dev(nb, dev), _dev(na, dev), 3, big_b[:hb.size], big_a[:ha.size]).cpu().numpy()
    assert np.array_equal(got, [EQUAL, BADREF, EQUAL])
    vals = [{"uvec": [(4, {"i": 1})], "sarr": [b"s", b"t"]}] * 3
    ca, cha = OBJ.stage(S.containertest, vals)
    cb, chb = OBJ.stage(S.containertest, vals)
    cst = compile_plan(S.containertest).stride
    ca = ca.copy()
    struct.pack_into("<QII", ca, cst + S.containertest.offsets["uvec"], cha.size - 23, 1, 0)  # 24-byte element
    cmar = _mar(S.containertest, dev)
    big_a = torch.zeros(cha.size + 4096, dtype=torch.uint8, device=dev)
    big_a[:cha.size] = _dev(cha, dev)
    got = cmar.compare(_dev(ca, dev), _dev(cb, dev), 3, big_a[:cha.size], _dev(chb, dev)).cpu().numpy()
    assert np.array_equal(got, [EQUAL, BADREF, EQUAL])


# --------------------------------------------------------------------- graph
def test_graph_capture_replays(dev):
    """A var plan with element subroutines, captured and replayed twice (the
    kernels keep no private memory: tests/test_compare_abi.py)."""
    b = F.batch("containertest")
    mar = _mar(S.containertest, dev)
    da, db, ha, hb = (_dev(x, dev) for x in (b.nat_a, b.nat_b, b.heap_a, b.heap_b))
    out = torch.full((b.n,), 99, dtype=torch.int8, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # the plan's tables go up outside the capture
        mar.launch_compare(da, db, b.n, out, ha, hb, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), b.cmp)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mar.launch_compare(da, db, b.n, out, ha, hb, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        out.fill_(99)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), b.cmp)


# ---------------------------------------------------------------- round trip
@pytest.mark.parametrize("name", ["recvar", "containertest"])
def test_round_trip_property(dev, name):
    """compare(x, decode(encode(x))) is EQUAL wherever x == x (a record that
    holds a NaN is unordered against itself), and value-equal coincides with
    byte-equal encodings (the reference's tests/autocheck.cc:31-38)."""
    n = 1024
    t = S.ALL[name]
    mar = _mar(t, dev)
    nat, heap = W.GENERATORS[name](n)
    self_cmp = CM.compare(mar.plan.cp, nat, heap, nat, heap, n)
    assert np.isin(self_cmp, [EQUAL, UNORDERED]).all() and (self_cmp == EQUAL).sum() >= n - 16
    dn, dh = _dev(nat, dev), _dev(heap, dev)
    enc = mar.encode(dn, n, dh)
    back, bheap = mar.decode(enc.xdr, n, enc.offsets)
    got = mar.compare(dn, back, n, dh, bheap).cpu().numpy()
    assert np.array_equal(got, self_cmp)
    again = mar.encode(back, n, bheap)
    assert torch.equal(again.xdr, enc.xdr)  # all equal <=> the two sides' bytes are
    # one record changed: not equal there, and its encoding alone differs
    st = mar.plan.stride
    changed = back.clone()
    first_ref = 16 if name == "recvar" else 0   # recvar.blob / containertest.uvec: {off, len or count}
    k = int(np.nonzero((nat.reshape(n, st)[:, first_ref + 8:first_ref + 12].view("<u4").reshape(-1) > 0)
                       & (self_cmp == EQUAL))[0][3])
    cnt = changed[k * st + first_ref + 8:k * st + first_ref + 12].view(torch.int32)
    cnt -= 1  # one byte / element fewer: the shorter one is less
    got = mar.compare(changed, dn, n, bheap, dh).cpu().numpy()
    want = self_cmp.copy()
    want[k] = LESS
    assert np.array_equal(got, want)
    offs = enc.offsets.cpu().numpy().astype(np.int64)
    x0 = enc.xdr.cpu().numpy()
    x1 = mar.encode(changed, n, bheap)
    o1 = x1.offsets.cpu().numpy().astype(np.int64)
    x1 = x1.xdr.cpu().numpy()
    for r in (k - 1, k, k + 1):
        same = np.array_equal(x0[offs[r]:offs[r + 1]], x1[o1[r]:o1[r + 1]])
        assert same == (r != k)
