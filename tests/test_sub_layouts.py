"""The element-subroutine kernels (csrc/sub_kernels.h's frame walks, the code
codegen.cpp generates for them, their launch logic in csrc/xdrgpu.hip) on the
layouts of oracle/x/subzoo.x: list nodes of every flat kind, wide and odd
strides, chains that do not end their record, a tail container in a union
arm, chains through an xvector, trees, nine nested container levels against
eight, elements at and past the inlined walkers' 64 bytes, two types that
contain each other.

CPU part: the layouts, described here with the xdr_types descriptors, are
held to what the REAL reference produced over genuine xdrc output
(tests/golden/sub.json, `make -C oracle sub`): the C++ layout, xdr_to_opaque,
check_xdr_depth, the stack limits, and xdr_from_opaque's exception on damaged
copies.  That pins the C restatement (oracle_bridge) on these layouts; the
larger GPU batches rest on it.  `classes()` restates the predicates that
choose a kernel path from the compiled ops, and the class table asserts that
the zoo holds every class of them: a layout that drifts to another path fails
here instead of passing on the wrong kernel.

GPU part: every layout, bit-exact against the fixture's 16 records and, for
larger batches, the restatement over the fixture's records tiled and followed
by generated records of the same shapes, in two stagings.
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import marshal as M
from xdrpp_amd import objects as OB
from xdrpp_amd.xdr_types import (Bool, Enum, Hyper, Int, OpaqueArray, Opaque, Pointer, String, Struct, Union, Void,
                                 XArray, XVector, _Scalar, _VarBytes, compile_plan)
import oracle_bridge as O
import verdict_model as V

gpu = pytest.mark.gpu
REF = "/root/reference"


@contextlib.contextmanager
def deep_recursion():
    """objects.stage, unstage, the value builder below and the comparison of
    their values recurse two or three times per list node (199 of them): a
    higher recursion limit for the length of such a call, then the session's
    own again."""
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 5000))
    try:
        yield
    finally:
        sys.setrecursionlimit(old)


# --------------------------------------------------------- oracle/x/subzoo.x
vtag = Enum("vtag", {"VNEG": -3, "VTWO": 2, "VBIG": 70000}, validate=True)
flatlist = Struct("flatlist")
flatlist.define([("b", Bool), ("e", vtag), ("h", Hyper), ("fx", OpaqueArray(5)), ("o", Opaque(20)),
                 ("s", String(12)), ("next", Pointer(flatlist))])
widelist = Struct("widelist")
widelist.define([("v", XArray(Hyper, 15)), ("a", String(9)), ("tail", Int), ("b", String(9)),
                 ("next", Pointer(widelist))])
oddlist = Struct("oddlist")
oddlist.define([("a", Int), ("s", String(7)), ("next", Pointer(oddlist))])
unode = Struct("unode")
utail = Union("utail", "k", Int, [([0], "", Void), ([1], "next", Pointer(unode)), ([2], "alt", String(8))])
unode.define([("s", String(6)), ("t", utail)])
vchain = Struct("vchain")
vchain.define([("s", String(8)), ("kids", XVector(vchain))])
tree = Struct("tree")
tree.define([("key", Int), ("s", String(6)), ("l", Pointer(tree)), ("r", Pointer(tree))])
_l = [None, Struct("l1", [("s", String(4))])]
for _k in range(2, 10):
    _l.append(Struct(f"l{_k}", [("v", XVector(_l[_k - 1])), ("i", Int)]))
e64 = Struct("e64", [("s", String(10)), ("h", XArray(Hyper, 6))])
e72 = Struct("e72", [("s", String(10)), ("h", XArray(Hyper, 7))])
ping, pong = Struct("ping"), Struct("pong")
ping.define([("s", String(5)), ("p", Pointer(pong))])
pong.define([("i", Int), ("q", Pointer(ping))])
ZOO = {t.name: t for t in [
    flatlist, widelist, oddlist,
    Struct("holder", [("a", Int), ("head", Pointer(flatlist)), ("after", String(10)), ("z", Int)]),
    Struct("twolists", [("a", Pointer(flatlist)), ("b", Pointer(flatlist))]),
    Struct("listvec", [("heads", XVector(flatlist))]),
    unode, vchain, tree,
    Struct("nest8", [("top", XVector(_l[8]))]),
    Struct("nest9", [("top", XVector(_l[9]))]),
    Struct("el64", [("v", XVector(e64))]),
    Struct("el72", [("v", XVector(e72))]),
    ping,
]}
NAMES = list(ZOO)
GPU_NAMES = NAMES
# the list, chain and tree types: every damaged copy of theirs is decoded on the device
LISTY = ["flatlist", "widelist", "oddlist", "holder", "twolists", "listvec", "unode", "vchain", "tree", "ping"]

# The predicates that choose a path, per type: (deep, packed, supported, list_vpc, tail_list, img_words,
# sub_tail of every VECTOR|SUB op in op order).  supported: codegen.cpp's, asked of plans that are not deep
# (None for the deep ones: they take the generated frame walks whatever it says); img_words: of the deep
# plans' frame walks (None: no frame walk is generated).  A literal table: classes() below must derive the
# same from the compiled ops, and the library's generated source must say the same.
TABLE = {
    "flatlist": (True, False, None, True, True, 20, (True,)),
    "widelist": (True, False, None, True, True, 32, (True,)),
    "oddlist":  (True, False, None, True, True, 12, (True,)),
    "holder":   (True, False, None, False, False, 20, (False, True)),
    "twolists": (True, False, None, False, False, 20, (False, True, True)),
    "listvec":  (True, False, None, False, False, 20, (True, True)),
    "unode":    (True, False, None, False, False, 12, (True,)),
    "vchain":   (True, False, None, False, False, 8, (True,)),
    "tree":     (True, False, None, False, False, 16, (False, True)),
    "nest8":    (False, True, True, False, False, None, (True,) + (False,) * 7),
    "nest9":    (True, False, None, False, False, 8, (True,) + (False,) * 8),
    "el64":     (False, True, True, False, False, None, (True,)),
    "el72":     (False, True, False, False, False, None, (True,)),
    "ping":     (True, False, None, False, False, 8, (True, True)),
}
K_MAX_IMG_WORDS = 32  # codegen.cpp kMaxImgWords
EUNSUPPORTED = -3     # XDRG_EUNSUPPORTED
NS = (1, 63, 64, 65, 257)


# ------------------------------------------------------------------ fixture
_gold_cache = []


def _fixture():
    if not _gold_cache:
        with open(os.path.join(GOLD, "sub.json")) as f:
            _gold_cache.append(json.load(f))
    return _gold_cache[0]


def _gold():
    return _fixture()["structs"]


_cps = {}


def cp_of(name):
    if name not in _cps:
        _cps[name] = compile_plan(ZOO[name])
    return _cps[name]


class SplitMix:
    """oracle/ref_util.hh's generator."""

    def __init__(self, s):
        self.s = s

    def __call__(self):
        m = (1 << 64) - 1
        self.s = (self.s + 0x9e3779b97f4a7c15) & m
        z = self.s
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & m
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & m
        return z ^ (z >> 31)


def unrle(counts):
    return [v for v, k in counts for _ in range(k)]


def build(t, g, counts):
    """The value oracle/ref_sub.cc's filler builds from a seed's generator
    `g` and the iterator `counts` (what every pointer, xvector and union
    takes, in wire order), as objects.stage takes it."""
    if t is Bool:
        return bool(g() & 1)
    if isinstance(t, Enum):
        tags = list(t.tags.values())
        return tags[g() % len(tags)]
    if isinstance(t, _Scalar):
        bits = 8 * t.size
        v = g() & ((1 << bits) - 1)
        return v - (1 << bits) if v >> (bits - 1) else v
    if isinstance(t, OpaqueArray):
        return bytes(g() & 0xff for _ in range(t.n))
    if isinstance(t, _VarBytes):
        n = g() % (t.max_len + 1)
        start = g() & 0xff
        step = (g() & 0xff) | 1
        return bytes((start + j * step) & 0xff for j in range(n))
    if isinstance(t, XArray):
        return [build(t.elem, g, counts) for _ in range(t.n)]
    if isinstance(t, Pointer):
        return build(t.elem, g, counts) if next(counts) else None
    if isinstance(t, XVector):
        return [build(t.elem, g, counts) for _ in range(next(counts))]
    if isinstance(t, Struct):
        return {f: build(ft, g, counts) for f, ft in t.fields}
    if isinstance(t, Union):
        disc = next(counts)
        arm = OB._arm(t, disc)
        return (disc, None if arm is Void else build(arm, g, counts))
    raise TypeError(t)


def value_of(name, seed, counts):
    it = iter(counts)
    with deep_recursion():
        v = build(ZOO[name], SplitMix(seed), it)
    assert next(it, None) is None
    return v


_values = {}


def gold_values(name):
    if name not in _values:
        _values[name] = [value_of(name, r["seed"], unrle(r["counts"])) for r in _gold()[name]["records"]]
    return _values[name]


def stage_alt(t, values):
    """objects.stage with another heap: a record's element arrays first, in
    the order the walk meets them, then all its payloads -- the nodes of a
    list lie a stride apart, where objects.stage puts each node's strings
    between it and the next."""
    stride = OB._align_up(t.size, t.align)
    native = bytearray(len(values) * stride)
    heap = OB._Heap()
    late = []

    def put(t, buf, off, v):
        if isinstance(t, _VarBytes):
            late.append((buf, off, v))
        elif isinstance(t, XArray):
            step = OB._align_up(t.elem.size, t.elem.align)
            for i, e in enumerate(v):
                put(t.elem, buf, off + i * step, e)
        elif isinstance(t, XVector):
            items = ([] if v is None else [v]) if isinstance(t, Pointer) else list(v)
            arr = heap.alloc(len(items) * t.stride, 8)
            struct.pack_into("<QII", buf, off, arr, len(items), 0)
            for i, e in enumerate(items):
                put(t.elem, heap.buf, arr + i * t.stride, e)
        elif isinstance(t, Struct):
            for fname, ft in t.fields:
                put(ft, buf, off + t.offsets[fname], v[fname])
        elif isinstance(t, Union):
            disc, val = v
            struct.pack_into("<i", buf, off, disc)
            arm = OB._arm(t, disc)
            if arm is not Void:
                put(arm, buf, off + t.arms_off, val)
        else:
            OB._put(t, buf, off, v, heap)

    for i, v in enumerate(values):
        with deep_recursion():
            put(t, native, i * stride, v)
        for buf, off, b in late:
            h = heap.alloc(len(b), 1)
            heap.buf[h:h + len(b)] = b
            struct.pack_into("<QII", buf, off, h, len(b), 0)
        late.clear()
    return np.frombuffer(bytes(native), np.uint8).copy(), np.frombuffer(bytes(heap.buf), np.uint8).copy()


def stage(t, values):
    with deep_recursion():
        return OB.stage(t, values)


def unstaged_equal(t, native, heap, n, values):
    """objects.unstage of n records gives `values`."""
    with deep_recursion():
        return OB.unstage(t, native, heap, n) == values


STAGERS = {"stage": stage, "alt": stage_alt}
_batches = {}


def batch_values(name):
    """257 records: the fixture's 16 twice over, then generated ones of the
    same shapes (record i has the counts of the fixture's record i % 16 and
    its own seed)."""
    key = (name, "values")
    if key not in _batches:
        recs = _gold()[name]["records"]
        gv = gold_values(name)
        _batches[key] = [gv[i % 16] for i in range(32)] + \
            [value_of(name, 0x5ab0000 + 977 * i, unrle(recs[i % 16]["counts"])) for i in range(32, max(NS))]
    return _batches[key]


def batch(name, n, how="stage"):
    """(values, native, heap, stream, offsets) of the first n records of the
    257-record batch staged by STAGERS[how] (one heap for every n: a prefix
    of the records reads a prefix of it); the stream is the restatement's."""
    key = (name, how)
    if key not in _batches:
        _batches[key] = STAGERS[how](ZOO[name], batch_values(name))
    nat, heap = _batches[key]
    nat = nat[:n * cp_of(name).stride]
    key = (name, how, n)
    if key not in _batches:
        want, offs = O.encode(cp_of(name), nat, n, heap)
        for a in (want, offs):
            a.flags.writeable = False
        _batches[key] = (want, offs)
    want, offs = _batches[key]
    return batch_values(name)[:n], nat, heap, want, offs


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record_ok(r, x):
    """`x` is the fixture's record `r`: the reference's own bytes."""
    if x.size != r["size"]:
        return False
    if "xdr" in r:
        return bytes(x).hex() == r["xdr"]
    return sha(x) == r["xdr_sha256"] and bytes(x[:32]).hex() == r["xdr_head"]


def pieces(x, offs):
    return [x[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def join(parts):
    offs = np.zeros(len(parts) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([p.size for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), offs


def damaged_copy(x, d):
    """A record's bytes with the fixture's damage [kind, offset, write,
    resize, exception]."""
    _, off, write, resize, _ = d
    w = np.frombuffer(bytes.fromhex(write), np.uint8)
    y = x.copy()
    y[off:off + w.size] = w
    if resize > 0:
        y = np.concatenate([y, np.zeros(resize, np.uint8)])
    elif resize < 0:
        y = y[:resize].copy()
    return y


# ======================================================================= CPU
def cxx_layout(t, cxx, offsets):
    """(size, alignment) of the C++ type xdrc generates for `t`: the staged
    layout with each 16-byte ref replaced by the container the reference
    keeps there (sizes from the fixture's header); offsets[name]: a struct's
    field offsets."""
    if isinstance(t, String):
        return tuple(cxx["xstring"])
    if isinstance(t, Opaque):
        return tuple(cxx["opaque_vec"])
    if isinstance(t, Pointer):
        return tuple(cxx["pointer"])
    if isinstance(t, XVector):
        return tuple(cxx["xvector"])
    if isinstance(t, XArray):
        s, a = cxx_layout(t.elem, cxx, offsets)
        return s * t.n, a
    if isinstance(t, Struct):
        off, al, offs = 0, 1, {}
        for f, ft in t.fields:
            s, a = cxx_layout(ft, cxx, offsets)
            off = (off + a - 1) // a * a
            offs[f] = off
            off += s
            al = max(al, a)
        offsets[t.name] = offs
        return (max(off, 1) + al - 1) // al * al, al
    if isinstance(t, Union):
        arms = [cxx_layout(a, cxx, offsets) for _, _, a in t.arms if a is not Void]
        al = max([4] + [a for _, a in arms])
        body = max([0] + [s for s, _ in arms])
        return ((4 + al - 1) // al * al + body + al - 1) // al * al, al
    return t.size, t.align


@pytest.mark.parametrize("name", NAMES)
def test_layout_equals_cxx(name):
    """The descriptors' fields, in order and with their scalar types, are the
    C++ struct's: laid out with the reference's containers in place of the
    16-byte refs they give its sizeof, alignof and every offsetof."""
    t, g = ZOO[name], _gold()[name]
    offsets = {}
    assert cxx_layout(t, _fixture()["cxx"], offsets) == (g["sizeof"], g["alignof"])
    assert offsets[name] == g["offsetof"]
    assert list(t.offsets) == list(g["offsetof"])
    assert cp_of(name).stride == t.size == M.Plan(cp_of(name)).stride


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_equal_subzoo_x(name):
    """The descriptors above are the types of oracle/x/subzoo.x (every enum
    of its namespace validated, as ref_sub.cc declares)."""
    import xdrc_front as xdrc
    from test_xdrc import same_plan
    sp = xdrc.load_file(os.path.join(ROOT, "oracle", "x", "subzoo.x"), validate_enums=("vtag",))
    assert same_plan(sp.plan(name), cp_of(name))


def test_front_end_refuses_a_cycle_by_value():
    """utail reaches unode through a pointer and parses (above); the same
    pair with the struct held by value has no layout, and compiling a plan
    of it is refused as recursive."""
    import xdrc_front as xdrc
    sp = xdrc.load("union u switch (int k) { case 1: s x; };\nstruct s { u t; };\n")
    for name in ("s", "u"):
        with pytest.raises(xdrc.XdrcError, match="recursive"):
            sp.plan(name)


@pytest.mark.skipif(not os.path.exists(f"{REF}/xdrpp/marshal.cc"), reason="reference tree absent")
def test_fixture_regenerates(tmp_path):
    """sub.json is what the reference produces today (empty diff)."""
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/ref_sub"], check=True)
    out = tmp_path / "s.json"
    subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_sub"), str(out)], check=True)
    assert out.read_bytes() == open(os.path.join(GOLD, "sub.json"), "rb").read()


def chain_len(v, link):
    n = 0
    while v is not None:
        n, v = n + 1, link(v)
    return n


def test_fixture_shapes():
    """The fixture's records have the issue's shapes: the node counts around
    kChainT = 32, the 64-node batch and kChainChunk, vchain's 3-element kids
    before and after logging starts, tree's spines and balanced trees, nests
    full to the bottom."""
    nodes = [0, 1, 2, 31, 32, 33, 34, 63, 64, 65, 66, 100, 129, 5, 96, 199]
    rooted = [max(k, 1) for k in nodes]
    for name in ("flatlist", "widelist", "oddlist"):
        assert [chain_len(v, lambda x: x["next"]) for v in gold_values(name)] == rooted
    assert [chain_len(v["head"], lambda x: x["next"]) for v in gold_values("holder")] == nodes
    two = gold_values("twolists")
    assert [chain_len(v["a"], lambda x: x["next"]) for v in two] == nodes
    assert [chain_len(v["b"], lambda x: x["next"]) for v in two] == nodes[5:] + nodes[:5]
    assert any(chain_len(v["a"], lambda x: x["next"]) > 33 < chain_len(v["b"], lambda x: x["next"]) for v in two)
    lv = [[chain_len(h, lambda x: x["next"]) for h in v["heads"]] for v in gold_values("listvec")]
    assert {len(x) for x in lv} == {0, 1, 2, 3, 4} and any(len(x) > 1 and min(x[:-1]) > 33 for x in lv)
    un = gold_values("unode")
    assert [chain_len(v, lambda x: x["t"][1] if x["t"][0] == 1 else None) for v in un] == rooted
    assert [chain_len(v, lambda x: x["p" if "p" in x else "q"]) for v in gold_values("ping")] == rooted
    vc = gold_values("vchain")
    spine = [chain_len(v, lambda x: x["kids"][-1] if x["kids"] else None) for v in vc]
    assert spine[:13] == rooted[:13] and spine[15] == 199
    for r, at in ((13, 5), (14, 40)):
        v = vc[r]
        for _ in range(at):
            assert len(v["kids"]) == 1
            v = v["kids"][0]
        assert len(v["kids"]) == 3
    tr = gold_values("tree")

    def depth(v):
        return 0 if v is None else 1 + max(depth(v["l"]), depth(v["r"]))

    def count(v):
        return 0 if v is None else 1 + count(v["l"]) + count(v["r"])
    assert [(depth(v), count(v)) for v in tr[:6]] == [(d, 2 ** d - 1) for d in range(1, 7)]
    assert chain_len(tr[6], lambda x: x["l"]) == 12 and chain_len(tr[9], lambda x: x["r"]) == 70
    for name, levels in (("nest8", 8), ("nest9", 9)):
        def bottom(v, k):  # a path down to an l1
            return k == 1 or any(bottom(e, k - 1) for e in v["v"])

        def sizes(v, k):
            return set() if k == 1 else {len(v["v"])}.union(*(sizes(e, k - 1) for e in v["v"]))
        recs = gold_values(name)
        assert sum(any(bottom(e, levels) for e in v["top"]) for v in recs) >= 2
        assert set().union(*({len(v["top"])} | set().union(*(sizes(e, levels) for e in v["top"]))
                             for v in recs)) == {0, 1, 3}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference(name):
    """The C restatement over the staged values: the reference's bytes,
    sizes, check_xdr_depth levels and both stack limits; its decode gives the
    values back (xdr_from_opaque's round trip held for every record), in
    either staging."""
    g = _gold()[name]["records"]
    cp = cp_of(name)
    vals = gold_values(name)
    for how in STAGERS:
        nat, heap = STAGERS[how](ZOO[name], vals)
        x, offs = O.encode(cp, nat, 16, heap)
        for r, p in zip(g, pieces(x, offs)):
            assert record_ok(r, p)
        assert list(O.sizes(cp, nat, 16, heap)) == [r["size"] for r in g]
        assert list(O.depths(cp, nat, 16, heap)) == [r["depth"] for r in g]
    assert all(r["round_trip"] for r in g)
    back, bheap = O.decode(cp, x, 16, offs)
    assert unstaged_equal(ZOO[name], back, bheap, 16, vals)
    s = cp.stride
    for i, r in enumerate(g):  # the smallest limits under which the record passes
        one = nat[i * s:(i + 1) * s]
        p = x[int(offs[i]):int(offs[i + 1])]
        o1 = np.array([0, p.size], dtype=np.uint64)
        O.encode(cp, one, 1, heap, stack_limit=r["put_limit"])
        O.decode(cp, p, 1, o1, stack_limit=r["get_limit"])
        with pytest.raises(O.OracleError) as e:
            O.encode(cp, one, 1, heap, stack_limit=r["put_limit"] - 1)
        assert e.value.code == A.ERR_STACK_PUT
        with pytest.raises(O.OracleError) as e:
            O.decode(cp, p, 1, o1, stack_limit=r["get_limit"] - 1)
        assert e.value.code == A.ERR_STACK_GET


EXC = {"xdr_should_be_zero": M.XdrShouldBeZero, "xdr_invariant_failed": M.XdrInvariantFailed,
       "xdr_overflow": M.XdrOverflow, "xdr_bad_message_size": M.XdrBadMessageSize,
       "xdr_bad_discriminant": M.XdrBadDiscriminant}
_host_plans = {}


def host_plan(name):
    if name not in _host_plans:
        _host_plans[name] = M.Plan(cp_of(name))
    return _host_plans[name]


def restatement_on(name, x, offs, n, **kw):
    """(code, record, op) of the restatement's failure on a stream, or None
    and its (native, heap)."""
    try:
        return None, O.decode(cp_of(name), x, n, offs, **kw)
    except O.OracleError as e:
        return (e.code, e.record, e.op), None


@pytest.mark.parametrize("name", NAMES)
def test_restatement_damaged_equals_reference(name):
    """Every damaged copy of every record: the restatement fails with the
    code of the reference's exception class.  Each listed copy must fail:
    the generator picked the byte.  The one exception is the reference's
    own: it reads any non-zero bool word as true (as the restatement does),
    so the "bool" copies decode, to the record with that bool set."""
    _, _, _, x, offs = batch(name, 16)
    for i, (r, p) in enumerate(zip(_gold()[name]["records"], pieces(x, offs))):
        for d in r["damaged"]:
            y = damaged_copy(p, d)
            err, out = restatement_on(name, y, np.array([0, y.size], dtype=np.uint64), 1)
            if d[0] == "bool":
                assert d[4] == "none" and err is None
                good, gheap = O.decode(cp_of(name), p, 1, np.array([0, p.size], dtype=np.uint64))
                # only the bool's byte differs, if it was false (it is true now), and the heap's copy of the word
                got = np.concatenate(out)
                differ = np.nonzero(got != np.concatenate([good, gheap]))[0]
                assert differ.size <= 2 and sorted(got[differ]) in ([2], [1, 2])
                continue
            assert d[4] in EXC and err is not None, (name, i, d)
            e = M.error_from(host_plan(name), A.XdrgError(code=err[0], record=err[1], op=err[2]))
            assert type(e) is EXC[d[4]], (name, i, d, err)


FLAT_CODES = {"enum": A.ERR_INVALID_ENUM, "pad_fixed": A.ERR_NONZERO_PAD, "pad": A.ERR_NONZERO_PAD,
              "count": A.ERR_POINTER_BOUND, "past": A.ERR_OVERFLOW_GET, "trailing": A.ERR_TRAILING,
              "truncated": A.ERR_OVERFLOW_GET}


def test_damage_kinds_cover_the_issue():
    """Every list type has every kind of damage its fields allow, and across
    flatlist's copies each code occurs: invalid enum, non-zero pad (of fx and
    of a payload), bad count, a length past the record, trailing bytes, a cut
    record.  (No code for a bad bool: the reference has no such exception.)"""
    z = _gold()
    kinds = {n: {d[0] for r in z[n]["records"] for d in r["damaged"]} for n in NAMES}
    common = {"pad", "past", "trailing", "truncated"}
    for n in NAMES:
        assert common - ({"past"} if n in ("tree", "nest8", "nest9", "el64", "el72") else set()) <= kinds[n], n
    for n in ("flatlist", "holder", "twolists", "listvec"):
        assert {"bool", "enum", "pad_fixed", "count"} <= kinds[n], n
    for n in ("widelist", "oddlist", "unode", "tree", "ping"):
        assert "count" in kinds[n], n
    _, _, _, x, offs = batch("flatlist", 16)
    seen = {}
    for r, p in zip(z["flatlist"]["records"], pieces(x, offs)):
        for d in r["damaged"]:
            if d[0] != "bool":
                y = damaged_copy(p, d)
                err, _ = restatement_on("flatlist", y, np.array([0, y.size], dtype=np.uint64), 1)
                seen.setdefault(d[0], set()).add(err[0])
    assert seen == {k: {c} for k, c in FLAT_CODES.items()}


# ------------------------------------------------------ which path a plan takes
def classes(cp):
    """The predicates that choose a path, from the compiled ops alone:
    plan.cpp's frames[] (deep, packed), codegen.cpp's supported(), tail_list()
    and img_words(), sub_kernels.h's list_vpc() and sub_tail()."""
    ops = cp.ops
    kind = [int(k) for k in ops["kind"]]
    n = len(kind)
    sub = [i for i in range(n) if kind[i] == A.OP_VECTOR and int(ops["flags"][i]) & A.F_SUB]
    flat = (A.OP_U32, A.OP_U64, A.OP_BOOL, A.OP_ENUM, A.OP_OPAQUE, A.OP_VAROPAQUE, A.OP_STRING)

    def sub_tail(pc):
        q = pc + 1
        while kind[q] == A.OP_JUMP:
            q = int(ops["arg0"][q])
        return kind[q] == A.OP_END

    # regions: the ops up to each END
    ends = [i for i in range(n) if kind[i] == A.OP_END]
    region = []
    for r, e in enumerate(ends):
        region += [r] * (e + 1 - len(region))
    frames, state = [0] * len(ends), [0] * len(ends)
    INF = float("inf")

    def visit(r):  # (the zoo's regions nest at most ten deep)
        state[r] = 1
        for i in range(ends[r - 1] + 1 if r else 0, ends[r]):
            if i not in sub:
                continue
            body = region[int(ops["arg4"][i])]
            if state[body] == 1:
                frames[r] = INF
                continue
            if state[body] == 0:
                visit(body)
            frames[r] = max(frames[r], frames[body] + 1)
        state[r] = 2
    visit(0)
    deep = frames[0] > A.SUB_FRAMES
    packed = any(k == A.OP_VECTOR for k in kind) and not deep
    supported = all(0 < int(ops["arg1"][i]) <= 64 and int(ops["arg1"][i]) % 4 == 0 for i in sub)
    # list_vpc
    pc = 0
    while pc < n and kind[pc] in flat:
        pc += 1
    ptr = A.F_SUB | A.F_POINTER
    list_vpc = (0 < pc < n and kind[pc] == A.OP_VECTOR and int(ops["flags"][pc]) & ptr == ptr and
                int(ops["arg0"][pc]) == 1 and int(ops["arg4"][pc]) == 0 and sub_tail(pc))
    # tail_list
    vpc = ends[0] - 1
    tail_list = (ends[0] > 0 and vpc in sub and int(ops["arg4"][vpc]) == 0 and int(ops["arg0"][vpc]) == 1 and
                 not any(i in sub for i in range(vpc)) and
                 not any(kind[i] == A.OP_JUMP and int(ops["arg0"][i]) > vpc for i in range(vpc)))
    img = min((max([int(ops["arg1"][i]) for i in sub] + [0]) + 15) // 16 * 4, K_MAX_IMG_WORDS)
    return (deep, packed, None if deep else supported, list_vpc, tail_list, img if deep else None,
            tuple(sub_tail(i) for i in sub))


@pytest.mark.parametrize("name", NAMES)
def test_classes_equal_the_table(name):
    assert classes(cp_of(name)) == TABLE[name]


def test_table_holds_every_class():
    """TABLE as a whole has every class the issue names: both values of every
    boolean predicate, image words below and at the limit, a tail container
    behind a JUMP, and each type's own class."""
    T = TABLE
    for col in (0, 1, 3, 4):
        assert {T[n][col] for n in NAMES} == {True, False}, col
    assert {T[n][2] for n in NAMES} == {True, False, None}
    assert {v for n in NAMES for v in T[n][6]} == {True, False}
    imgs = {T[n][5] for n in NAMES} - {None}
    assert K_MAX_IMG_WORDS in imgs and min(imgs) < K_MAX_IMG_WORDS

    def only(pred):
        return {n for n in NAMES if pred(T[n])}
    lists = only(lambda c: c[3])
    assert lists == {"flatlist", "widelist", "oddlist"} == only(lambda c: c[4])
    assert only(lambda c: c[5] == K_MAX_IMG_WORDS) == {"widelist"}         # fields inside and past the image
    assert only(lambda c: c[3] and c[5] % 4 == 0 and c[5] * 4 - 8 == 40) == {"oddlist"}  # stride 8 mod 16
    assert only(lambda c: c[3] and c[5] == 20) == {"flatlist"}
    # chains that do not end their record: a container that is no tail before one that is
    assert only(lambda c: c[0] and c[6] == (False, True)) == {"holder", "tree"}
    assert only(lambda c: c[6] == (False, True, True)) == {"twolists"}
    assert only(lambda c: c[6] == (True, True) and c[5] == 20) == {"listvec"}
    # a tail container that is not a list (through the union's JUMP; an xvector; two regions)
    assert only(lambda c: c[0] and not c[3] and c[6] == (True,)) == {"unode", "vchain"}
    assert T["unode"][5] != T["vchain"][5]
    assert only(lambda c: c[6] == (True, True) and c[5] == 8) == {"ping"}  # ping's tail enters pong's region, whose
    assert int(cp_of("ping").ops["arg4"][1]) != 0 and int(cp_of("ping").ops["arg4"][-2]) == 0  # tail comes back
    # plan.deep without recursion on either side of XDRG_SUB_FRAMES
    assert only(lambda c: len(c[6]) == A.SUB_FRAMES and not c[0] and c[1]) == {"nest8"}
    assert only(lambda c: len(c[6]) == A.SUB_FRAMES + 1 and c[0] and not c[1]) == {"nest9"}
    # supported()'s stride bound
    assert only(lambda c: c[2] is True and len(c[6]) == 1) == {"el64"}
    assert only(lambda c: c[2] is False) == {"el72"}
    assert cp_of("el64").ops["arg1"][0] == 64 and cp_of("el72").ops["arg1"][0] == 72
    assert cp_of("oddlist").stride % 16 == 8 and cp_of("widelist").stride > 128
    # the union's JUMP lies between unode's pointer and its END
    ops = cp_of("unode").ops
    v = int(np.nonzero(ops["kind"] == A.OP_VECTOR)[0][0])
    assert ops["kind"][v + 1] == A.OP_JUMP


def source(plan):
    L = A.lib()
    n = C.c_size_t(0)
    assert L.xdrg_plan_kernel_source(plan.handle, None, 0, C.byref(n)) == A.OK
    buf = C.create_string_buffer(n.value + 1)
    assert L.xdrg_plan_kernel_source(plan.handle, buf, n.value + 1, C.byref(n)) == A.OK
    return buf.value.decode()


def info_of(plan):
    info = A.XdrgPlanInfo()
    A.check(A.lib().xdrg_plan_get_info(plan.handle, C.byref(info)), "xdrg_plan_get_info")
    return info


@pytest.mark.parametrize("name", NAMES)
def test_generated_source_is_the_expected_path(name):
    """The library agrees with the table from the host: the frame walks
    (xdrg_spec_sub_size) exactly for the deep plans, with the table's image
    words; the list's index parse exactly for the tail lists; no frame walk
    in the inlined walkers of the supported plans; no source at all for an
    element past 64 bytes; and hiprtc (or the kernel cache) yields a code
    object, which touches no device."""
    deep, packed, supported, _, tail_list, img, _ = TABLE[name]
    p = M.Plan(ZOO[name])
    L = A.lib()
    if supported is False:  # no generated code: the library's interpreted kernels, under either setting
        n = C.c_size_t(0)
        assert L.xdrg_plan_kernel_source(p.handle, None, 0, C.byref(n)) == EUNSUPPORTED
        assert L.xdrg_plan_build_kernels(p.handle) == EUNSUPPORTED and info_of(p).specialized == 0
        return
    src = source(p)
    assert ("xdrg_spec_sub_size" in src) == deep
    assert (f"kImgWords = {img}u" in src) == deep
    assert ("// a node of the list" in src) == tail_list
    if not deep:
        assert "xdrg_spec_sub_" not in src and "packed() const { return true; }" in src
    rc = L.xdrg_plan_build_kernels(p.handle)
    assert rc == A.OK, L.xdrg_last_hip_error().decode()
    assert info_of(p).specialized == 1


# ======================================================================= GPU
def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


def i64(offs, dev):
    return to_dev(np.asarray(offs).astype(np.int64), dev)


_mars = {}


def marshaler(dev, name, spec):
    """One plan and marshaler per layout and `specialize` value."""
    key = (name, spec)
    if key not in _mars:
        _mars[key] = M.Marshaler(M.Plan(ZOO[name], {"specialize": spec}), dev)
    return _mars[key]


def device_on(mar, x, offs, n, dev, **kw):
    """(code, record, op) of the device decode's failure, or None and its
    (native, heap) -- restatement_on's counterpart."""
    try:
        nat, heap = mar.decode(to_dev(x, dev), n, i64(offs, dev), **kw)
    except M.XdrRuntimeError as e:
        return (e.code, e.record, 0xFFFFFFFF if e.op is None else e.op), None  # (None: a record-level error)
    return None, (nat.cpu().numpy(), heap.cpu().numpy())


def same_decode(name, mar, x, offs, n, dev, **kw):
    """The device decodes a stream as the restatement does: the same native
    records and heap, or the same code, record and op."""
    want, wout = restatement_on(name, x, offs, n, **kw)
    got, gout = device_on(mar, x, offs, n, dev, **kw)
    assert got == want, (name, got, want)
    if want is None:
        assert np.array_equal(gout[0], wout[0]) and np.array_equal(gout[1], wout[1]), name
    return want


def verify_frames(name):
    """The frames xdrg_verify needs for each fixture record, from the value:
    only tree's left pointers count (a one-element tail container -- every
    link of the other chains, through a union arm's JUMP too, and tree's
    right pointer -- opens none there; nest9 opens nine)."""
    def lefts(v, cur=0):
        return cur if v is None else max(cur, lefts(v["l"], cur + 1) if v["l"] else 0, lefts(v["r"], cur))
    if name != "tree":
        return [0] * 16
    with deep_recursion():
        return [lefts(v) for v in gold_values("tree")]


def check_verdicts(name, mar, x, offs, dev):
    """xdrg_verify's per-record verdicts over the fixture's 16 records (clean
    or damaged) are the restatement's, every one.  Only a record that really
    nests past XDRG_INDEX_FRAMES through containers that are no tails may
    come back undecided (XDRG_ERR_INDEX_LONG, include/xdrgpu.h): tree's
    zigzag and random tree, 20 and 25 left pointers deep, and nothing else in
    the zoo.  Returns the device's verdicts."""
    spans = np.stack([offs[:-1], offs[1:]], axis=1).astype(np.int64)
    want = V.oracle_verdicts(cp_of(name), x, spans)
    v, bad = mar.verify(to_dev(x, dev), i64(offs, dev))
    got = v.cpu().numpy().view(np.uint32)
    frames = verify_frames(name)
    assert [r for r in range(16) if frames[r] > A.INDEX_FRAMES] == ([14, 15] if name == "tree" else [])
    for r in range(16):
        ok = got[r] == want[r] or (frames[r] > A.INDEX_FRAMES and got[r] & 0xFF == A.ERR_INDEX_LONG)
        assert ok, (name, r, hex(got[r]), hex(want[r]))
    assert bad == np.count_nonzero(got)
    return got


@gpu
@pytest.mark.parametrize("spec", [1, 0])
@pytest.mark.parametrize("name", GPU_NAMES)
def test_fixture_records_gpu(dev, name, spec):
    """The fixture's 16 records: the reference's own bytes and offsets out,
    its sizes and depths, its values back (natives and heap the
    restatement's), the same through record-marked messages and through the
    device's own record index, and clean verdicts."""
    g = _gold()[name]["records"]
    cp = cp_of(name)
    vals, nat, heap, want, woffs = batch(name, 16)
    mar = marshaler(dev, name, spec)
    dn, dh = to_dev(nat, dev), to_dev(heap, dev)
    res = mar.encode(dn, 16, dh)
    got, offs = res.xdr.cpu().numpy(), res.offsets.cpu().numpy().astype(np.uint64)
    assert np.array_equal(offs, woffs) and np.array_equal(got, want)
    for r, p in zip(g, pieces(got, offs)):
        assert record_ok(r, p)
    assert list(mar.serial_sizes(dn, 16, heap=dh).cpu().numpy()) == [r["size"] for r in g]
    assert list(mar.record_depths(dn, 16, dh).cpu().numpy()) == [r["depth"] for r in g]
    assert same_decode(name, mar, want, woffs, 16, dev) is None
    back, bheap = mar.decode(res.xdr, 16, res.offsets)
    assert unstaged_equal(ZOO[name], back.cpu().numpy(), bheap.cpu().numpy(), 16, vals)
    # record-marked messages
    mwant, moffs = O.encode_msgs(cp, nat, 16, heap)
    m = mar.encode_msgs(dn, 16, dh)
    assert np.array_equal(m.xdr.cpu().numpy(), mwant)
    mnat, mheap = mar.decode_msgs(m.xdr)
    onat, oheap = O.decode_msgs(cp, mwant, 16, moffs)
    assert np.array_equal(mnat.cpu().numpy(), onat) and np.array_equal(mheap.cpu().numpy(), oheap)
    # no offsets: the record index (on the device, or the host walk it hands deep streams to)
    inat, iheap = mar.decode(res.xdr, 16)
    assert np.array_equal(inat.cpu().numpy(), back.cpu().numpy())
    assert np.array_equal(iheap.cpu().numpy(), bheap.cpu().numpy())
    deep_ones = [r for r, f in enumerate(verify_frames(name)) if f > A.INDEX_FRAMES]
    assert not np.delete(check_verdicts(name, mar, want, woffs, dev), deep_ones).any()
    assert info_of(mar.plan).specialized == (spec if TABLE[name][2] is not False else 0)


@gpu
@pytest.mark.parametrize("spec", [1, 0])
@pytest.mark.parametrize("name", GPU_NAMES)
def test_batches_gpu(dev, name, spec):
    """Batches of 1 to 257 records in both stagings -- objects.stage's, where
    a node's strings lie between it and the next node (the chain pass's
    guess of the spacing misses), and one with the nodes a stride apart --
    encode to the restatement's bytes and offsets and decode to its natives
    and heap."""
    mar = marshaler(dev, name, spec)
    for n in NS:
        for how in STAGERS:
            _, nat, heap, want, woffs = batch(name, n, how)
            res = mar.encode(to_dev(nat, dev), n, to_dev(heap, dev))
            assert np.array_equal(res.offsets.cpu().numpy().astype(np.uint64), woffs), (name, n, how)
            assert np.array_equal(res.xdr.cpu().numpy(), want), (name, n, how)
        assert np.array_equal(want, batch(name, n)[3])  # (either staging: the same stream)
        assert same_decode(name, mar, want, woffs, n, dev) is None


@gpu
@pytest.mark.parametrize("spec", [1, 0])
@pytest.mark.parametrize("name", LISTY)
def test_damaged_copies_gpu(dev, name, spec):
    """Every damaged copy of the fixture, one at a time in its own record of
    the 16-record stream: the restatement's record, op and code (the "bool"
    copies: its decode); then every record damaged at once, by the kinds in
    turn: decode reports the first, verify each record's own verdict."""
    mar = marshaler(dev, name, spec)
    g = _gold()[name]["records"]
    _, _, _, x, offs = batch(name, 16)
    parts = pieces(x, offs)
    failed = 0
    for i, r in enumerate(g):
        for d in r["damaged"]:
            bx, boffs = join(parts[:i] + [damaged_copy(parts[i], d)] + parts[i + 1:])
            err = same_decode(name, mar, bx, boffs, 16, dev)
            assert (err is None) == (d[0] == "bool") and (err is None or err[1] == i), (name, i, d, err)
            failed += err is not None
    assert failed >= 16 * 3
    every = [damaged_copy(p, r["damaged"][i % len(r["damaged"])]) for i, (r, p) in enumerate(zip(g, parts))]
    bx, boffs = join(every)
    assert same_decode(name, mar, bx, boffs, 16, dev) is not None
    assert np.count_nonzero(check_verdicts(name, mar, bx, boffs, dev)) >= 12


def flat_node_offsets(v):
    """Where each node of a flatlist record starts on the wire."""
    at, p = [], 0
    while v is not None:
        at.append(p)
        p += 4 + 4 + 8 + 8 + 4 + (len(v["o"]) + 3 & ~3) + 4 + (len(v["s"]) + 3 & ~3) + 4
        v = v["next"]
    return at, p


@gpu
@pytest.mark.parametrize("spec", [1, 0])
def test_flatlist_long_record_value_checks(dev, spec):
    """A flatlist of 200 nodes between two short records: a long record of
    more than one 8 KiB block, decoded by the wave pass in batches of 64 nodes.
    One change at a time in node 3 (the first batch), 64 (the first of the
    second), 65 and 199 (the last): an invalid enum and a non-zero fx pad
    fail at the restatement's record, op and code (the batch's value checks
    send the record to the walk from its start); a bool word of 2 decodes,
    as the reference reads it."""
    recs = _gold()["flatlist"]["records"]
    vals = [gold_values("flatlist")[2], value_of("flatlist", 0xf1a7, [1] * 199 + [0]), gold_values("flatlist")[5]]
    nat, heap = stage(flatlist, vals)
    x, offs = O.encode(cp_of("flatlist"), nat, 3, heap)
    at, size = flat_node_offsets(vals[1])
    assert len(at) == 200 and size == int(offs[2] - offs[1]) > 8192 and recs[2]["size"] == int(offs[1])
    mar = marshaler(dev, "flatlist", spec)
    assert same_decode("flatlist", mar, x, offs, 3, dev) is None
    codes = set()
    for node in (3, 64, 65, 199):
        a = int(offs[1]) + at[node]
        for kind, pos, w in (("bool", a, [0, 0, 0, 2]), ("enum", a + 4, [0, 0, 0, 3]), ("pad_fixed", a + 21, [1])):
            bx = x.copy()
            bx[pos:pos + len(w)] = w
            err = same_decode("flatlist", mar, bx, offs, 3, dev)
            assert (err is None) == (kind == "bool"), (node, kind, err)
            if err is not None:
                assert err[1] == 1
                codes.add(err[0])
    assert codes == {A.ERR_INVALID_ENUM, A.ERR_NONZERO_PAD}


def same_encode_error(name, mar, nat, heap, n, dev, exc, **kw):
    """An encode that fails does so at the restatement's record and op."""
    with pytest.raises(O.OracleError) as oe:
        O.encode(cp_of(name), nat, n, heap, **{{"capacity": "cap"}.get(k, k): v for k, v in kw.items()})
    with pytest.raises(exc) as e:
        mar.encode(to_dev(nat, dev), n, to_dev(heap, dev), **kw)
    assert (e.value.record, 0xFFFFFFFF if e.value.op is None else e.value.op) == (oe.value.record, oe.value.op), \
        (name, kw)
    return oe.value


@gpu
@pytest.mark.parametrize("spec", [1, 0])
def test_limits_inside_gpu(dev, spec):
    """Stack limits that end inside a logged chain (holder's 63- and 100-node
    lists, past kChainT = 32 nodes), inside tree's left spine of 12 (within
    and past the 8 register frames) and inside nest9's ninth level, and a
    capacity that ends in holder.after, behind the chain's close: the
    reference's first failing record, the restatement's op, on encode and
    decode."""
    for name, limits in (("holder", (100, 150)), ("tree", (14, 20)), ("nest9", None)):
        g = _gold()[name]["records"]
        _, nat, heap, x, offs = batch(name, 16)
        mar = marshaler(dev, name, spec)
        if limits is None:  # one level short of the record that is full to the bottom (record 1)
            assert g[1]["put_limit"] == g[1]["get_limit"] == max(r["put_limit"] for r in g)
            limits = (g[1]["put_limit"] - 1,)
        for L in limits:
            put = next(i for i, r in enumerate(g) if r["put_limit"] > L)
            get = next(i for i, r in enumerate(g) if r["get_limit"] > L)
            if name == "holder":  # the record the limit ends in has a logged chain
                assert put == get == {100: 7, 150: 11}[L]
                assert chain_len(gold_values(name)[put]["head"], lambda v: v["next"]) == {100: 63, 150: 100}[L]
            elif name == "tree":  # record 6: the left spine of 12, two levels a node
                assert put == get == 6 and g[6]["put_limit"] == 24
            else:
                assert put == get == 1
            e = same_encode_error(name, mar, nat, heap, 16, dev, M.XdrStackOverflow, stack_limit=L,
                                  capacity=int(offs[-1]))
            assert e.record == put
            err = same_decode(name, mar, x, offs, 16, dev, stack_limit=L)
            assert err is not None and err[:2] == (A.ERR_STACK_GET, get)
    vals = [dict(v) for v in gold_values("holder")]
    vals[11]["after"] = b"0123456789"
    nat, heap = stage(ZOO["holder"], vals)
    x, offs = O.encode(cp_of("holder"), nat, 16, heap)
    cap = int(offs[12]) - 4 - 8  # inside `after`'s bytes
    e = same_encode_error("holder", marshaler(dev, "holder", spec), nat, heap, 16, dev, M.XdrOverflow, capacity=cap)
    ops = cp_of("holder").ops
    assert e.record == 11 and ops["kind"][e.op] == A.OP_STRING and e.op > int(np.nonzero(ops["kind"] == A.OP_VECTOR)[0][0])


@gpu
@pytest.mark.parametrize("spec", [1, 0])
def test_wave_pass_gpu(dev, spec):
    """Long records (4 KiB or more: the decode's wave pass) of plans that are
    not one list: nest9, nine frames against the wave's, and listvec with
    100-node lists (chains in elements that are not the last), among short
    ones: the restatement's natives and heap."""
    # nest9: 3 elements at the levels named, 1 at the others
    def nest_counts(levels, wide):
        if levels == 0:
            return []
        n = 3 if levels in wide else 1
        return [n] + nest_counts(levels - 1, wide) * n
    cases = {
        "nest9": [unrle(_gold()["nest9"]["records"][2]["counts"]), nest_counts(9, {9, 5, 4, 3, 2, 1}), [0],
                  nest_counts(9, {6, 5, 4, 3, 2, 1}), nest_counts(9, set())],
        "listvec": [[1, 0], [3] + ([1] * 99 + [0]) * 3, [0], [2] + ([1] * 99 + [0]) + [0], [2, 0] + [1] * 99 + [0]],
    }
    for name, shapes in cases.items():
        vals = [value_of(name, 0x3a7e + i, c) for i, c in enumerate(shapes)]
        n = len(vals)
        for how in STAGERS:
            nat, heap = STAGERS[how](ZOO[name], vals)
            x, offs = O.encode(cp_of(name), nat, n, heap)
            sizes = np.diff(offs.astype(np.int64))
            assert (sizes >= 4096).sum() >= 2 and (sizes < 4096).sum() >= 2, (name, sizes)
            mar = marshaler(dev, name, spec)
            res = mar.encode(to_dev(nat, dev), n, to_dev(heap, dev))
            assert np.array_equal(res.xdr.cpu().numpy(), x), (name, how)
        assert same_decode(name, mar, x, offs, n, dev) is None
        back, bheap = mar.decode(res.xdr, n, res.offsets)
        assert unstaged_equal(ZOO[name], back.cpu().numpy(), bheap.cpu().numpy(), n, vals)


@gpu
@pytest.mark.parametrize("spec", [1, 0])
def test_oddlist_last_node_ends_the_heap(dev, spec):
    """oddlist's nodes are 40 bytes, 8 mod 16: a node's register image (three
    16-byte loads) reaches 8 bytes past it.  With an empty string in the last
    node, that node is the last thing in the staged heap, and the image's
    last load would pass heap_len: the walk's heap-end branch.  Lists around
    the chain log's threshold, alone and in a batch."""
    def lst(k, r):
        v = None
        for i in reversed(range(k)):
            v = {"a": 1000 * r + i, "s": b"" if i == k - 1 else bytes([97 + (i + r) % 26] * ((i + r) % 8)), "next": v}
        return v
    mar = marshaler(dev, "oddlist", spec)
    for lens in ([2], [33], [70], [1, 2, 31, 32, 33, 34, 64, 65, 130]):
        vals = [lst(k, r) for r, k in enumerate(lens)]
        nat, heap = stage(oddlist, vals)
        if lens[-1] > 1:  # the last node ends the heap, and its image (kImgWords words) reaches past heap_len
            assert bytes(heap[-40:-36]) == struct.pack("<i", 1000 * (len(lens) - 1) + lens[-1] - 1)
            assert cp_of("oddlist").stride == 40 and heap.size - 40 + 4 * TABLE["oddlist"][5] > heap.size
        n = len(vals)
        x, offs = O.encode(cp_of("oddlist"), nat, n, heap)
        res = mar.encode(to_dev(nat, dev), n, to_dev(heap, dev))
        assert np.array_equal(res.xdr.cpu().numpy(), x), lens
        assert list(mar.serial_sizes(to_dev(nat, dev), n, heap=to_dev(heap, dev)).cpu().numpy()) == \
            list(np.diff(offs.astype(np.int64))), lens
        assert same_decode("oddlist", mar, x, offs, n, dev) is None
