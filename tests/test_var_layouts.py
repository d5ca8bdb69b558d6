"""The var-record kernels (var_kernels.h var_encode_body / var_decode_body,
the walkers codegen.cpp emits, the path choice of var_encode / var_decode in
csrc/xdrgpu.hip) on the layouts of oracle/x/varzoo.x: every chunk-map slot
count, a fifth payload, word lists at and past their limits, every register
load shape, records longer than an image or a window, records of 4 bytes.

CPU part: the layouts, described here with the xdr_types descriptors, are
held to what the REAL reference produced over genuine xdrc output
(tests/golden/var.json, `make -C oracle var`): the C++ layout, xdr_to_opaque,
xdr_from_opaque and its exception on damaged streams.  That pins the C
restatement (oracle_bridge) on these layouts; the larger GPU batches rest on
it.  `paths()` restates which walker codegen.cpp emits for a layout, and the
class table asserts that the zoo holds every class of them: a layout that
drifts to another path fails here instead of passing on the wrong kernel.

GPU part: every layout, bit-exact against the fixture's 16 records and, for
larger batches, the restatement over the fixture's records tiled twice and
followed by generated records of the same length cycle.
"""
import ctypes as C
import hashlib
import json
import os
import re
import struct

import numpy as np
import pytest

from conftest import GOLD, ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import marshal as M
from xdrpp_amd import objects as OB
from xdrpp_amd.xdr_types import (Bool, Enum, Hyper, Int, Opaque, OpaqueArray, Pointer, String, Struct, Union,
                                 Void, XArray, _Scalar, _VarBytes, compile_plan)
import oracle_bridge as O

gpu = pytest.mark.gpu
REF = "/root/reference"

# -------------------------------------------------------- oracle/x/varzoo.x
vtag = Enum("vtag", {"VNEG": -3, "VTWO": 2, "VBIG": 70000}, validate=True)
arm3 = Struct("arm3", [("x", Opaque(9)), ("y", String(11)), ("z", Opaque(33))])
armu = Union("armu", "which", Int, [([0], "", Void), ([1], "a", Opaque(20)), ([2], "t", arm3)])
ZOO = {t.name: t for t in [
    Struct("one", [("o", Opaque(40))]),
    Struct("three", [("a", Opaque(20)), ("b", String(33)), ("i", Int), ("c", Opaque(17))]),
    Struct("four", [("a", Opaque(16)), ("h", Hyper), ("b", String(31)), ("c", Opaque(5)), ("d", String(48))]),
    Struct("five", [("a", String(9)), ("b", Opaque(24)), ("i", Int), ("c", Opaque(15)), ("d", String(32)),
                    ("e", Opaque(7))]),
    Struct("str8", [(f"s{k}", String(12)) for k in range(8)]),
    Struct("str9", [(f"s{k}", String(12)) for k in range(9)]),
    Struct("w22", [("v", XArray(Int, 21)), ("o", Opaque(30))]),
    Struct("w24", [("v", XArray(Int, 23)), ("o", Opaque(30))]),
    Struct("wide136", [("v", XArray(Hyper, 15)), ("o", Opaque(30))]),
    Struct("long9k", [("i", Int), ("o", Opaque(9000)), ("s", String(20))]),
    Struct("unbounded", [("i", Int), ("o", Opaque()), ("s", String())]),
    Struct("tiny", [("o", Opaque(3))]),
    Struct("mixed", [("b0", Bool), ("fx", OpaqueArray(5)), ("o", Opaque(30)), ("p", Pointer(String(10))),
                     ("b1", Bool)]),
    Struct("armslots", [("u", armu), ("tail", String(13))]),
    Struct("venum", [("e", vtag), ("s", String(7))]),
]}
NAMES = list(ZOO)

# What codegen.cpp emits for each layout: (KMAX, NW, kWords, CMAX, `c.copy(src, len)` sites, PRE variants).
# A literal table: paths() below must derive the same from the type, and the generated source must say the same.
TABLE = {
    "one":       (1, 4, 1, 4096, 0, True),
    "three":     (3, 14, 4, 4096, 0, True),
    "four":      (4, 18, 6, 4096, 0, True),
    "five":      (4, 22, 0, 8192, 1, False),
    "str8":      (4, 32, 0, 8192, 4, False),
    "str9":      (4, 0, 0, 8192, 5, False),
    "w22":       (1, 26, 22, 4096, 0, True),
    "w24":       (1, 28, 0, 8192, 0, False),
    "wide136":   (1, 0, 0, 8192, 0, False),
    "long9k":    (2, 10, 3, 4096, 0, True),
    "unbounded": (2, 10, 0, 8192, 2, False),
    "tiny":      (1, 4, 1, 4096, 0, True),
    "mixed":     (1, 12, 0, 8192, 1, False),
    "armslots":  (4, 18, 5, 4096, 0, True),
    "venum":     (1, 6, 2, 4096, 0, True),
}
WORD_LIST = [n for n in NAMES if TABLE[n][2]]

# codegen.cpp's constants
SLOT_MAX, MAX_LIST_WORDS, REG_RECORD_BYTES, SLOT_BYTES = 4, 24, 128, 1 << 30
UNBOUNDED_AS = 1000  # the bound oracle/ref_var.cc's length cycle gives an unbounded field
CYCLE = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, -1, -2]  # (-1, -2: B - 1, B)
NS = (1, 16, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def zoo_gold():
    return _gold()


_gold_cache = []


def _fixture():
    if not _gold_cache:
        with open(os.path.join(GOLD, "var.json")) as f:
            _gold_cache.append(json.load(f))
    return _gold_cache[0]


def _gold():
    return _fixture()["structs"]


_cps = {}


def cp_of(name):
    if name not in _cps:
        _cps[name] = compile_plan(ZOO[name])
    return _cps[name]


def ramp(start, step, n):
    return ((start + np.arange(n, dtype=np.uint64) * step) & 0xff).astype(np.uint8).tobytes()


def to_value(t, j):
    """A fixture value as objects.stage takes it."""
    if t is Bool:
        return bool(j)
    if isinstance(t, (_Scalar, Enum)):
        return int(j)
    if isinstance(t, OpaqueArray):
        return bytes.fromhex(j)
    if isinstance(t, _VarBytes):
        return ramp(*j)
    if isinstance(t, XArray):
        return [to_value(t.elem, e) for e in j]
    if isinstance(t, Pointer):
        return None if j is None else to_value(t.elem, j)
    if isinstance(t, Struct):
        return {f: to_value(ft, j[f]) for f, ft in t.fields}
    if isinstance(t, Union):
        arm = OB._arm(t, j[0])
        return (j[0], None if arm is Void else to_value(arm, j[1]))
    raise TypeError(t)


def gold_values(name):
    return [to_value(ZOO[name], j) for j in _gold()[name]["values"]]


def cycle_len(i, k, B):
    B = min(B, UNBOUNDED_AS)
    c = CYCLE[(i + 5 * k) % 16]
    return B - (c == -1) if c < 0 else min(c, B)


def gen_value(t, i, rng, k=None):
    """Record i of a generated batch: payload k has the cycle's length
    (shifted by one per 16 records, so the fields' lengths meet in new
    combinations), unions go round their arms, pointers are set in odd
    records."""
    k = [0] if k is None else k
    if t is Bool:
        return bool(rng.integers(0, 2))
    if isinstance(t, Enum):
        return int(rng.choice(sorted(t.tags.values())))
    if isinstance(t, _Scalar):
        bits = 8 * t.size
        v = int.from_bytes(rng.integers(0, 256, t.size, dtype=np.uint8).tobytes(), "little")
        return v - (1 << bits) if not t.name.startswith("unsigned") and v >= 1 << (bits - 1) else v
    if isinstance(t, OpaqueArray):
        return rng.integers(0, 256, t.n, dtype=np.uint8).tobytes()
    if isinstance(t, _VarBytes):
        n = cycle_len(i + i // 16, k[0], t.max_len)
        k[0] += 1
        return ramp(int(rng.integers(0, 256)), int(rng.integers(0, 256)) | 1, n)
    if isinstance(t, XArray):
        return [gen_value(t.elem, i, rng, k) for _ in range(t.n)]
    if isinstance(t, Pointer):
        return gen_value(t.elem, i, rng, k) if i & 1 else None
    if isinstance(t, Struct):
        return {f: gen_value(ft, i, rng, k) for f, ft in t.fields}
    if isinstance(t, Union):
        disc = t.arms[i % len(t.arms)][0][0]
        arm = OB._arm(t, disc)
        return (disc, None if arm is Void else gen_value(arm, i, rng, k))
    raise TypeError(t)


_batches = {}


def batch(name, n, patch=None):
    """(values, native, heap, stream, offsets) of an n-record batch: the
    fixture's 16 records twice over, then generated ones; the stream is the
    restatement's.  `patch`: {record: value} replacing records."""
    key = (name, n)
    if patch is None and key in _batches:
        return _batches[key]
    t = ZOO[name]
    rng = np.random.default_rng([n, len(name)])
    gv = gold_values(name)
    vals = [gv[i % 16] for i in range(min(n, 32))] + [gen_value(t, i, rng) for i in range(32, n)]
    for r, v in (patch or {}).items():
        vals[r] = v
    nat, heap = OB.stage(t, vals)
    want, offs = O.encode(cp_of(name), nat, n, heap)
    for a in (nat, heap, want, offs):
        a.flags.writeable = False
    out = (vals, nat, heap, want, offs)
    if patch is None:
        _batches[key] = out
    return out


def unhex(s):
    return np.frombuffer(bytes.fromhex(s), dtype=np.uint8).copy()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ======================================================================= CPU
def cxx_layout(t, cxx):
    """(size, alignment) of the C++ type xdrc generates for `t`: the staged
    layout with each xdrg_bytes_ref replaced by the container the reference
    keeps there (std::vector, std::string, std::unique_ptr; sizes from the
    fixture's header)."""
    if isinstance(t, String):
        return tuple(cxx["xstring"])
    if isinstance(t, Opaque):
        return tuple(cxx["opaque_vec"])
    if isinstance(t, Pointer):
        return tuple(cxx["pointer"])
    if isinstance(t, XArray):
        s, a = cxx_layout(t.elem, cxx)
        return s * t.n, a
    if isinstance(t, Struct):
        off, al, offs = 0, 1, {}
        for f, ft in t.fields:
            s, a = cxx_layout(ft, cxx)
            off = (off + a - 1) // a * a
            offs[f] = off
            off += s
            al = max(al, a)
        t_size = (max(off, 1) + al - 1) // al * al
        cxx.setdefault("_offsets", {})[t.name] = offs
        return t_size, al
    if isinstance(t, Union):
        arms = [cxx_layout(a, cxx) for _, _, a in t.arms if a is not Void]
        al = max([4] + [a for _, a in arms])
        body = max([0] + [s for s, _ in arms])
        return ((4 + al - 1) // al * al + body + al - 1) // al * al, al
    return t.size, t.align


@pytest.mark.parametrize("name", NAMES)
def test_layout_equals_cxx(name):
    """The descriptors' fields, in order and with their scalar types, are the
    C++ struct's: laid out with the reference's containers in place of the
    16-byte refs they give its sizeof, alignof and every offsetof; and the
    staged layout (compile_plan, objects.stage) is that layout with 16-byte,
    8-aligned refs."""
    cxx = dict(_fixture()["cxx"])
    t, g = ZOO[name], _gold()[name]
    size, align = cxx_layout(t, cxx)
    assert (size, align) == (g["sizeof"], g["alignof"])
    assert cxx["_offsets"][name] == g["offsetof"]
    assert list(t.offsets) == list(g["offsetof"])
    cp = cp_of(name)
    p = M.Plan(cp)
    assert cp.stride == t.size == p.stride and cp.is_var
    nat, _ = OB.stage(t, gold_values(name))
    assert nat.size == 16 * cp.stride
    assert p.max_record_bytes >= max(g["sizes"])  # (xdrg_plan_get_info's bound holds for every record)


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_equal_varzoo_x(name):
    """The descriptors above are the types of oracle/x/varzoo.x (every enum
    of its namespace validated, as ref_var.cc declares)."""
    import xdrc_front as xdrc
    from test_xdrc import same_plan
    sp = xdrc.load_file(os.path.join(ROOT, "oracle", "x", "varzoo.x"), validate_enums=("vtag",))
    assert same_plan(sp.plan(name), cp_of(name))


@pytest.mark.skipif(not os.path.exists(f"{REF}/xdrpp/marshal.cc"), reason="reference tree absent")
def test_fixture_regenerates(tmp_path):
    """var.json is what the reference produces today (empty diff)."""
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/ref_var"], check=True)
    out = tmp_path / "v.json"
    subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_var"), str(out)], check=True)
    assert out.read_bytes() == open(os.path.join(GOLD, "var.json"), "rb").read()


def test_fixture_records_follow_the_cycle(zoo_gold):
    """The fixture's lengths are the cycle's: `four` runs through all 16
    empty / non-empty combinations, long9k has the lengths around the 4 and
    8 KiB images, armslots takes every arm, tiny has heaps under 16 bytes."""
    four = [tuple(bool(len(v[f])) for f in "abcd") for v in gold_values("four")]
    assert len(set(four)) == 16
    assert {0, 4091, 4092, 4093, 8191, 8192, 8999, 9000} <= {len(v["o"]) for v in gold_values("long9k")}
    assert {v["u"][0] for v in gold_values("armslots")} == {0, 1, 2}
    assert {len(v["o"]) for v in gold_values("tiny")} == {0, 1, 2, 3}
    assert max(len(v["o"]) for v in gold_values("unbounded")) == UNBOUNDED_AS
    for name in ("one", "three", "five", "str9", "w22"):
        t = ZOO[name]
        var = [f for f, ft in t.fields if isinstance(ft, _VarBytes)]
        for i, v in enumerate(gold_values(name)):
            assert [len(v[f]) for f in var] == [cycle_len(i, k, dict(t.fields)[f].max_len) for k, f in enumerate(var)]
    assert zoo_gold["mixed"]["values"][1]["p"] is not None and zoo_gold["mixed"]["values"][0]["p"] is None


def gold_stream_ok(g, x):
    if "xdr" in g:
        return bytes(x).hex() == g["xdr"]
    return sha(x) == g["xdr_sha256"] and bytes(x[:64]).hex() == g["xdr_head"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_encode_equals_reference(zoo_gold, name):
    g = zoo_gold[name]
    _, nat, heap, x, offs = batch(name, 16)
    assert gold_stream_ok(g, x)
    assert list(np.diff(offs)) == g["sizes"]
    assert list(O.sizes(cp_of(name), nat, 16, heap)) == g["sizes"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_decode_equals_reference(zoo_gold, name):
    g = zoo_gold[name]
    assert g["decoded"] == "values"  # xdr_from_opaque gave every record's values back
    vals, _, _, x, offs = batch(name, 16)
    nat, heap = O.decode(cp_of(name), x, 16, offs)
    assert OB.unstage(ZOO[name], nat, heap, 16) == vals


EXC = {"xdr_should_be_zero": M.XdrShouldBeZero, "xdr_invariant_failed": M.XdrInvariantFailed,
       "xdr_overflow": M.XdrOverflow, "xdr_bad_message_size": M.XdrBadMessageSize,
       "xdr_bad_discriminant": M.XdrBadDiscriminant}


def damaged_cases():
    z = _gold()
    return [(n, k) for n in z for k in range(len(z[n]["damaged"]))]


def damage(x, offs, d, record=None):
    """The stream with the fixture's damage `d` in `record` (default: the
    fixture's own record), and its offsets."""
    r = d["at_record"] if record is None else record
    x = x.copy()
    w = unhex(d["write"])
    p = int(offs[r]) + d["offset"]
    x[p:p + w.size] = w
    offs = offs.copy()
    if d["resize"] > 0:
        x = np.concatenate([x, np.zeros(d["resize"], np.uint8)])
    elif d["resize"] < 0:
        x = x[:d["resize"]].copy()
    offs[-1] = x.size
    return x, offs


_host_plans = {}


def check_verdict(cp, err, d, record):
    """A (code, record, op) is the reference's verdict `d`: its record, its
    exception class and its what()."""
    code, rec, op = err
    assert rec == record
    if id(cp) not in _host_plans:
        _host_plans[id(cp)] = M.Plan(cp)
    e = M.error_from(_host_plans[id(cp)], A.XdrgError(code=code, record=rec, op=op))
    assert type(e) is EXC[d["exception"]] and str(e) == d["what"]


@pytest.mark.parametrize("name,k", damaged_cases())
def test_restatement_damaged_equals_reference(zoo_gold, name, k):
    """The reference's first failing record, exception class and what()."""
    d = zoo_gold[name]["damaged"][k]
    assert d["record"] == d["at_record"]
    _, _, _, x, offs = batch(name, 16)
    bad, boffs = damage(x, offs, d)
    with pytest.raises(O.OracleError) as ei:
        O.decode(cp_of(name), bad, 16, boffs)
    e = ei.value
    check_verdict(cp_of(name), (e.code, e.record, e.op), d, d["record"])


def test_damage_kinds_cover_the_issue(zoo_gold):
    kinds = {n: {d["kind"] for d in g["damaged"]} for n, g in zoo_gold.items()}
    for n in NAMES:
        assert {"pad", "past", "truncated", "trailing"} <= kinds[n], n
        assert ("bound" in kinds[n]) == (n != "unbounded")
    assert "discriminant" in kinds["armslots"] and "enum" in kinds["venum"] and "pad_fixed" in kinds["mixed"]
    whats = {d["what"] for g in zoo_gold.values() for d in g["damaged"]}
    assert {"xvector overflow", "xstring overflow", "Non-zero padding bytes encountered",
            "insufficient buffer space in xdr_generic_get", "unmarshaling did not consume whole message",
            "bad value of which in armu", "Invalid enum value"} == whats


# ------------------------------------------------------ which walker is emitted
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


def walk_shape(t, slot=0):
    """(slots, scalar words, copy sites, what rules a word list out) of the
    encode walk over `t` starting at chunk-map slot `slot`, along the longest
    path through the unions (codegen.cpp enc_block, restated from the type
    alone)."""
    if isinstance(t, OpaqueArray):
        return slot, (t.n + 3) // 4, 0, set()
    if isinstance(t, (_Scalar, Enum)):
        return slot, 2 if t.size == 8 else 1, 0, set()
    if isinstance(t, _VarBytes):
        if slot >= SLOT_MAX:
            return slot, 1, 1, {"copy"}  # the fifth payload: copied by its lane
        if t.max_len > SLOT_BYTES:
            return slot + 1, 1, 1, {"unbounded"}  # a payload that may pass the slot limit
        return slot + 1, 1, 0, set()
    if isinstance(t, XArray):
        t = Struct("", [(str(i), t.elem) for i in range(t.n)])
    if isinstance(t, Struct):
        words, copies, why = 0, 0, set()
        for _, ft in t.fields:
            slot, w, c, y = walk_shape(ft, slot)
            words, copies, why = words + w, copies + c, why | y
        return slot, words, copies, why
    if isinstance(t, Union):
        arms = [a for _, _, a in t.arms if a is not Void]
        if t.default is not None and t.default[1] is not Void:
            arms.append(t.default[1])
        got = [walk_shape(a, slot) for a in arms] or [(slot, 0, 0, set())]
        return (max(g[0] for g in got), 1 + max(g[1] for g in got), sum(g[2] for g in got),
                set().union(*(g[3] for g in got)))
    if hasattr(t, "elem"):  # xvector / pointer: a count word; its elements' payloads are copied
        c = 0 if t.elem.fixed_wire is not None else walk_shape(t.elem, SLOT_MAX)[2]
        return slot, 1, c, {"container"}
    raise TypeError(t)


def paths(plan, t):
    """What codegen.cpp emits for a plan, from xdrg_plan_get_info, the type
    and the constants 4 (slots), 24 (list words) and 128 (register records):
    kWords, the template arguments of every var_encode_body it instantiates,
    the number of `c.copy(src, len)` sites, whether the walk-first kernels
    (xdrg_spec_encode_pre / _lb) exist, whether var_encode launches them at
    the default image size, and what rules the word list out."""
    info = info_of(plan)
    stride, max_rec = info.native_stride, int(info.max_record_bytes)
    slots, words, copies, why = walk_shape(t)
    regs = stride <= REG_RECORD_BYTES and stride % 4 == 0
    if not why and not regs:
        why = {"stride"}
    if not why and words + 1 > MAX_LIST_WORDS:
        why = {"words"}
    if not why and 4 * (words + 1) > stride:
        why = {"tile"}
    kwords = 0 if why else words
    nw = stride // 4 if regs else 0
    base = f"{max(1, slots)}, 4, {nw}, {4096 if kwords else 8192}u"
    image = min(4096, (64 * max(max_rec, 16) + 31) & ~15)
    return {"kWords": kwords, "encode": [base] + ([f"{base}, 2", f"{base}, 1"] if kwords else []),
            "copies": copies, "pre": kwords > 0, "pre_runs": kwords > 0 and 256 * (kwords + 1) <= image,
            "why_no_list": why}


@pytest.mark.parametrize("name", NAMES)
def test_generated_source_is_the_expected_walker(name):
    """xdrg_plan_kernel_source agrees with paths() and with the literal
    table: the template arguments, kWords, the copy sites, PRE."""
    t = ZOO[name]
    p = M.Plan(t)
    want = paths(p, t)
    kmax, nw, kwords, cmax, copies, pre = TABLE[name]
    base = f"{kmax}, 4, {nw}, {cmax}u"
    assert want["encode"] == [base] + ([f"{base}, 2", f"{base}, 1"] if pre else [])
    assert (want["kWords"], want["copies"], want["pre"]) == (kwords, copies, pre)
    src = source(p)
    assert re.findall(r"var_encode_body<plan_walk, ([^>]*)>", src) == want["encode"]
    assert re.findall(r"kWords = (\d+)u", src) == [str(kwords)]
    assert src.count("c.copy(src, len)") == copies
    assert ("xdrg_spec_encode_pre" in src) == pre == ("xdrg_spec_encode_lb" in src)
    # the size and decode walks load the record the same way (NW)
    assert re.findall(r"var_size_body<plan_walk, (\d+)>", src) == [str(nw)]
    assert re.findall(r"var_decode_body<plan_walk, (?:true|false), true, (\d+)>", src) == [str(nw)] * 2
    for k in range(SLOT_MAX + 1):
        assert (f"c.template slot<{k}>" in src) == (k < kmax)


def test_zoo_holds_every_class():
    """Every class of walker is in the zoo at least once (from paths(),
    which test_generated_source_is_the_expected_walker holds to the
    source)."""
    ps = {n: paths(M.Plan(ZOO[n]), ZOO[n]) for n in NAMES}
    kmax = {n: int(ps[n]["encode"][0].split(", ")[0]) for n in NAMES}
    nw = {n: int(ps[n]["encode"][0].split(", ")[2]) for n in NAMES}
    assert {kmax[n] for n in NAMES} == {1, 2, 3, 4}
    assert {kmax[n] for n in WORD_LIST} == {1, 2, 3, 4}  # ... each on the walk-first kernel too
    assert any(v and v % 4 == 0 for v in nw.values())          # load_rec: 16-byte loads
    assert any(v % 4 == 2 for v in nw.values())                # 8-byte loads
    assert any(v == 0 for v in nw.values())                    # no register record
    assert ps["w22"]["kWords"] == 22 and ps["w22"]["pre"]      # a word list at 22 words (23 with the mark)
    assert ps["w24"]["kWords"] == 0 and ps["w24"]["why_no_list"] == {"words"}  # none at 24 (25 with the mark)
    assert ps["five"]["why_no_list"] == {"copy"} and ps["unbounded"]["why_no_list"] == {"unbounded"}
    assert ps["wide136"]["why_no_list"] == {"stride"} and "container" in ps["mixed"]["why_no_list"]
    assert all(ps[n]["why_no_list"] == set() for n in WORD_LIST)
    assert {ps[n]["pre"] for n in NAMES} == {True, False}
    # a word list whose walk-first kernel var_encode never launches: 256 * 23 words pass the 4 KiB image
    assert ps["w22"]["pre"] and not ps["w22"]["pre_runs"]
    assert all(ps[n]["pre_runs"] for n in WORD_LIST if n != "w22")
    # the interpreter's KMAX (1, 2 or 4) from the same slot counts
    assert {1 if k <= 1 else 2 if k <= 2 else 4 for k in kmax.values()} == {1, 2, 4}
    # five payloads or more: off the image kernel
    assert {n for n in NAMES if "copy" in ps[n]["why_no_list"] and n != "mixed"} == {"five", "str8", "str9"}


@pytest.mark.parametrize("name", NAMES)
def test_source_compiles_for_gfx950(name):
    """hiprtc (or the kernel cache) yields a code object for every layout;
    compiling touches no device."""
    p = M.Plan(ZOO[name])
    L = A.lib()
    rc = L.xdrg_plan_build_kernels(p.handle)
    assert rc == A.OK, L.xdrg_last_hip_error().decode()
    assert info_of(p).specialized == 1


def linear(cp):
    """plan.cpp's linear plans (the walk-free size pass k_size_linear): no
    union, jump or container, at most 8 payload fields."""
    kinds = [int(o["kind"]) for o in cp.ops]
    var = sum(k in (A.OP_VAROPAQUE, A.OP_STRING) for k in kinds)
    return var <= 8 and not any(k in (A.OP_UNION, A.OP_JUMP, A.OP_VECTOR) for k in kinds)


def test_linear_size_pass_boundary():
    """str8 is the last plan the linear size pass takes, str9 the first it
    does not: the plans for which size_linear does and does not change the
    size pass (test_size_linear_gpu runs both under 1, 0 and -1)."""
    assert linear(cp_of("str8")) and not linear(cp_of("str9"))
    assert not linear(cp_of("armslots")) and not linear(cp_of("mixed")) and linear(cp_of("one"))


# ======================================================================= GPU
def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


def heap_dev(heap, dev):
    return to_dev(heap, dev) if heap is not None and heap.size else None


def one_pass(mar, nat, n, heap, cap, dev, msgs=False):
    """xdrg_encode (msgs: xdrg_encode_msgs) into a buffer of `cap` bytes
    filled with 0xEE, a 64-byte guard after it: (bytes up to the total,
    offsets, error or None, status)."""
    import torch
    out = torch.full((max(cap, 4) + 64,), 0xEE, dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    mar.status.init(s)
    if msgs:
        mar.launch_encode_msgs(to_dev(nat, dev), n, out[:cap], offs, heap=heap_dev(heap, dev), stream=s)
    else:
        mar.launch_encode(to_dev(nat, dev), n, out[:cap], heap=heap_dev(heap, dev), offsets=offs, stream=s)
    e = mar.status.read(s)
    assert bool((out[cap:] == 0xEE).all()), "encode wrote past its capacity"
    err = None if e.code == 0 else (e.code, e.record, e.op)
    got = out[:e.total_bytes] if err is None else out[:cap]
    return got.cpu().numpy(), offs.cpu().numpy().view(np.uint64), err, e


_mars = {}


def marshaler(dev, name, opts):
    """One plan and marshaler per layout and option set."""
    key = (name, tuple(sorted(opts.items())))
    if key not in _mars:
        _mars[key] = M.Marshaler(M.Plan(ZOO[name], opts), dev)
    return _mars[key]


def check_encode(dev, name, opts, n, nat=None, heap=None, want=None, woffs=None, two_halves=False):
    """One encode under `opts`: the bytes (pad bytes included: the buffer is
    born 0xEE and the expected stream has zeros there), the offsets, the
    total, the guard."""
    if nat is None:
        _, nat, heap, want, woffs = batch(name, n)
    mar = marshaler(dev, name, opts)
    got, offs, err, e = one_pass(mar, nat, n, heap, want.size, dev)
    assert err is None, (name, opts, n, err)
    assert e.total_bytes == want.size, (name, opts, n)
    assert np.array_equal(got, want), (name, opts, n)
    assert np.array_equal(offs, woffs), (name, opts, n)
    # the generated walker was built and loaded where it is asked for (no quiet fall to the interpreter)
    assert info_of(mar.plan).specialized == (opts.get("specialize", 1) and not opts.get("var_encode_kernel", 0))
    if two_halves:  # xdrg_encode_sizes, then xdrg_encode_sized
        res = mar.encode(to_dev(nat, dev), n, heap_dev(heap, dev))
        assert np.array_equal(res.xdr.cpu().numpy(), want), (name, opts, n, "two halves")
        assert np.array_equal(res.offsets.cpu().numpy().view(np.uint64), woffs), (name, opts, n, "two halves")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_fixture_records_gpu(dev, zoo_gold, name):
    """The fixture's 16 records: the reference's own bytes out, its values
    back."""
    g = zoo_gold[name]
    vals, nat, heap, want, woffs = batch(name, 16)
    assert gold_stream_ok(g, want)
    mar = M.Marshaler(M.Plan(ZOO[name]), dev)
    res = mar.encode(to_dev(nat, dev), 16, heap_dev(heap, dev))
    assert gold_stream_ok(g, res.xdr.cpu().numpy())
    assert list(np.diff(res.offsets.cpu().numpy().view(np.uint64))) == g["sizes"]
    back, bheap = mar.decode(res.xdr, 16, res.offsets)
    assert OB.unstage(ZOO[name], back.cpu().numpy(), bheap.cpu().numpy(), 16) == vals


def spec_settings(name):
    streams = (-1, 1, 0) if name in WORD_LIST else (-1,)
    return [{"specialize": 1, "enc_stream": st, "image_bytes": img} for st in streams for img in (-1, 256)]


INTERP = [{"specialize": 0, "var_encode_kernel": k, "enc_unroll": u, "image_bytes": img}
          for k in (0, 1, 3) for u in (4, 8, 16) for img in (-1, 256)]


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_encode_specialized(dev, name):
    """The generated walker: the walk-first kernel over the scan (enc_stream
    -1), over the look-back (1) and the per-window walk (0) for word-list
    layouts; the default image and a 256-byte one (every record longer than
    256 bytes then spans several rounds); one pass and the two halves."""
    for opts in spec_settings(name):
        for n in NS:
            check_encode(dev, name, opts, n, two_halves=True)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_encode_interpreter(dev, name):
    """The plan interpreter: kernel choice 0 (auto), 1 (one lane per record)
    and 3 (the image kernel, KMAX 1, 2 or 4; five payloads or more must not
    run it and come out right when it is asked for), every unroll, both
    images."""
    for opts in INTERP:
        for n in NS:
            check_encode(dev, name, opts, n, two_halves=opts["enc_unroll"] == 8)


@gpu
@pytest.mark.parametrize("linear_opt", [1, 0, -1])
@pytest.mark.parametrize("name", ["str8", "str9"])
def test_size_linear_gpu(dev, name, linear_opt):
    """The walk-free size pass on the last plan it takes and the first it
    does not: xdr_size of every record and the same encode, generated walker
    and interpreter."""
    for spec in (1, 0):
        opts = {"size_linear": linear_opt, "specialize": spec}
        for n in NS:
            _, nat, heap, want, woffs = batch(name, n)
            mar = marshaler(dev, name, opts)
            sz = mar.serial_sizes(to_dev(nat, dev), n, heap=heap_dev(heap, dev)).cpu().numpy().astype(np.uint64)
            assert np.array_equal(sz, np.diff(woffs)), (name, opts, n)
            check_encode(dev, name, opts, n, two_halves=True)


MSG_LAYOUTS = ["one", "four", "five"]  # 1 slot, 4 slots, a fifth payload


@gpu
@pytest.mark.parametrize("spec", [1, 0])
@pytest.mark.parametrize("name", MSG_LAYOUTS)
def test_messages_gpu(dev, name, spec):
    """xdrg_encode_msgs and xdrg_decode_msgs (each record behind its mark)."""
    for n in NS:
        vals, nat, heap, _, _ = batch(name, n)
        cp = cp_of(name)
        want, woffs = O.encode_msgs(cp, nat, n, heap)
        for opts in ({"specialize": spec}, {"specialize": spec, "image_bytes": 256, "window_bytes": 256}):
            mar = marshaler(dev, name, opts)
            got, offs, err, _ = one_pass(mar, nat, n, heap, want.size, dev, msgs=True)
            assert err is None and np.array_equal(got, want) and np.array_equal(offs, woffs), (name, opts, n)
            back, bheap = mar.decode_msgs(to_dev(want, dev), n, to_dev(woffs.view(np.int64), dev))
            o_nat, o_heap = O.decode_msgs(cp, want, n, woffs)
            assert np.array_equal(back.cpu().numpy(), o_nat), (name, opts, n)
            assert np.array_equal(bheap.cpu().numpy(), o_heap), (name, opts, n)
            assert OB.unstage(ZOO[name], back.cpu().numpy(), bheap.cpu().numpy(), n) == vals


# ---- heap shapes
HEAP_LAYOUTS = ["one", "three", "four", "five"]


def var_fields(t):
    return [(f, t.offsets[f]) for f, ft in t.fields if isinstance(ft, _VarBytes)]


def reheap(name, nat, heap, n, seed):
    """The same records with every payload moved: a shuffled order, gaps,
    and piece j placed at a source address of residue j mod 16."""
    t = ZOO[name]
    rec = nat.reshape(n, t.size).copy()
    rng = np.random.default_rng(seed)
    pieces = []
    for r in range(n):
        for _, off in var_fields(t):
            src, ln, _ = struct.unpack_from("<QII", rec[r], off)
            pieces.append((r, off, heap[src:src + ln]))
    out = bytearray()
    residues = set()
    for j, i in enumerate(rng.permutation(len(pieces))):
        r, off, b = pieces[i]
        out += rng.integers(0, 256, 16 * int(rng.integers(0, 3)) + (j - len(out)) % 16, dtype=np.uint8).tobytes()
        residues.add(len(out) % 16)
        rec[r, off:off + 8] = np.frombuffer(struct.pack("<Q", len(out)), np.uint8)
        out += b.tobytes()
    assert residues == set(range(16)) or len(pieces) < 16
    return rec.reshape(-1), np.frombuffer(bytes(out), np.uint8).copy()


HEAP_OPTS = [{"specialize": 1}, {"specialize": 1, "enc_stream": 1}, {"specialize": 1, "enc_stream": 0},
             {"specialize": 0, "var_encode_kernel": 3}, {"specialize": 0, "var_encode_kernel": 1},
             {"specialize": 1, "image_bytes": 256}, {"specialize": 0, "var_encode_kernel": 3, "image_bytes": 256}]


@gpu
@pytest.mark.parametrize("name", HEAP_LAYOUTS)
def test_heap_shapes(dev, name):
    """Where the payloads lie: in record order (the last payload then ends
    exactly at heap_len), shuffled with gaps so that their sources fall on
    every residue mod 16, with 1..15 bytes after the last payload, and with
    heap_len cut inside the last payload (bytes past it read 0; the
    restatement is given the zeros)."""
    cp = cp_of(name)
    t = ZOO[name]
    cuts = 0
    for n in (16, 65, 257):
        vals, nat, heap, want, woffs = batch(name, n)
        # the last payload of the record-order heap ends at heap_len
        ends = [struct.unpack_from("<QII", nat, r * t.size + off)[:2] for r in range(n) for _, off in var_fields(t)]
        assert max(s + ln for s, ln in ends) == heap.size
        shuf_nat, shuf_heap = reheap(name, nat, heap, n, n)
        swant, soffs = O.encode(cp, shuf_nat, n, shuf_heap)
        assert np.array_equal(swant, want) and np.array_equal(soffs, woffs)
        last = max(ln for s, ln in ends if s + ln == heap.size)
        for opts in HEAP_OPTS:
            check_encode(dev, name, opts, n)  # record order
            check_encode(dev, name, opts, n, shuf_nat, shuf_heap, want, woffs)
            for cut in sorted({1, min(5, last), last} - {0}):  # heap_len inside the last payload
                short = heap[:heap.size - cut]
                cwant, coffs = O.encode(cp, nat, n, np.concatenate([short, np.zeros(cut + 64, np.uint8)]))
                check_encode(dev, name, opts, n, nat, short, cwant, coffs)
                cuts += 1
        for tail in range(1, 16):  # the last payload ends 1..15 bytes before heap_len
            longer = np.concatenate([heap, np.full(tail, 0xC3, np.uint8)])
            for opts in HEAP_OPTS[:4]:
                check_encode(dev, name, opts, n, nat, longer, want, woffs)
    assert cuts


@gpu
@pytest.mark.parametrize("ln", [0, 1, 2, 3])
def test_tiny_heap(dev, ln):
    """One record of tiny with a heap of 0..3 bytes (heap_tail16's byte
    path), and 65 records whose whole heap is under 16 bytes."""
    t = ZOO["tiny"]
    cp = cp_of("tiny")
    for vals in ([{"o": ramp(7, 3, ln)}], [{"o": ramp(r, 5, ln if r % 32 == 0 else 0)} for r in range(65)]):
        n = len(vals)
        nat, heap = OB.stage(t, vals)
        assert heap.size < 16
        want, woffs = O.encode(cp, nat, n, heap)
        for opts in HEAP_OPTS:
            check_encode(dev, "tiny", opts, n, nat, heap, want, woffs)


# ---- decode
def dec_settings():
    return [{"specialize": sp, "var_decode_kernel": k, "window_bytes": w, "dec_readahead": ra}
            for sp in (1, 0) for k in (0, 1, 2) for w in (-1, 256) for ra in (0, 1)]


def run_decode(mar, p, x, offs, n, dev, zero_copy):
    """(native, heap) of a raw xdrg_decode; zero_copy: heap_out is the
    stream's own buffer (refs into the stream)."""
    import torch
    H = p.decode_heap_bytes(x.size)
    s = torch.cuda.current_stream().cuda_stream
    native = torch.zeros(max(n, 1) * p.stride, dtype=torch.uint8, device=dev)
    if zero_copy:
        hout = torch.zeros(max(H, x.size, 4), dtype=torch.uint8, device=dev)
        hout[:x.size] = to_dev(x, dev)
        xin = hout[:x.size]
    else:
        hout = torch.zeros(max(H, 4), dtype=torch.uint8, device=dev)
        xin = to_dev(x, dev)
    mar.status.init(s)
    mar.launch_decode(xin, n, native, offsets=to_dev(offs.view(np.int64), dev), heap_out=hout, stream=s)
    mar.check(s)
    return native.cpu().numpy(), hout[:H].cpu().numpy()


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_decode_settings(dev, name):
    """Good streams under every decode setting: the generated walker and the
    interpreter, kernel choice 0, 1 (a lane per record) and 2 (the window
    kernel), the default window and a 256-byte one (most records then start
    past it), with and without the read-ahead, into a heap copy and
    zero-copy: the restatement's native bytes and heap, the batch's values."""
    cp = cp_of(name)
    t = ZOO[name]
    for n in NS:
        vals, _, _, x, offs = batch(name, n)
        o_nat, o_heap = O.decode(cp, x, n, offs)
        assert OB.unstage(t, o_nat, o_heap, n) == vals
        for opts in dec_settings():
            mar = marshaler(dev, name, opts)
            for zc in (False, True):
                nat, heap = run_decode(mar, mar.plan, x, offs, n, dev, zc)
                assert np.array_equal(nat, o_nat), (name, opts, n, zc)
                assert np.array_equal(heap, o_heap), (name, opts, n, zc)
            # the generated walker runs under kernel choice 0 only, and was built and loaded there
            assert info_of(mar.plan).specialized == (opts["specialize"] and not opts["var_decode_kernel"])


# ---- damaged streams
DAMAGE_AT = (0, 63, 64, 256)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_damaged_streams_gpu(dev, zoo_gold, name):
    """Every damage case of the fixture in record 0, 63, 64 and 256 of 257
    (truncated and trailing streams: the last record), and in 64 and 256
    together (the lowest record is reported): the restatement's code, record
    and op, which are the reference's exception and what().  The damaged
    record is the fixture's own record of that case, so the damage sits
    where the reference saw it."""
    import torch
    n = 257
    cp = cp_of(name)
    t = ZOO[name]
    gv = gold_values(name)
    plans = [M.Plan(t, o) for o in ({"specialize": 1}, {"specialize": 0}, {"specialize": 1, "window_bytes": 256},
                                    {"specialize": 0, "var_decode_kernel": 1})]
    mars = [M.Marshaler(p, dev) for p in plans]
    for d in zoo_gold[name]["damaged"]:
        at = (256,) if d["resize"] else DAMAGE_AT
        vals, nat, heap, x, offs = batch(name, n, patch={r: gv[d["at_record"]] for r in at})
        cases = [(r,) for r in at] + ([(64, 256)] if not d["resize"] else [])
        for rs in cases:
            bad, boffs = x, offs
            for r in rs:
                bad, boffs = damage(bad, boffs, d, r)
            with pytest.raises(O.OracleError) as oi:
                O.decode(cp, bad, n, boffs)
            want = (oi.value.code, oi.value.record, oi.value.op)
            check_verdict(cp, want, d, rs[0])
            for p, mar in zip(plans, mars):
                native = torch.zeros(n * p.stride, dtype=torch.uint8, device=dev)
                hout = torch.zeros(max(p.decode_heap_bytes(bad.size), 4), dtype=torch.uint8, device=dev)
                s = torch.cuda.current_stream().cuda_stream
                mar.status.init(s)
                mar.launch_decode(to_dev(bad, dev), n, native, offsets=to_dev(boffs.view(np.int64), dev),
                                  heap_out=hout, stream=s)
                e = mar.status.read(s)
                assert (e.code, e.record, e.op) == want, (name, d["kind"], rs)


# ---- capacity
@gpu
@pytest.mark.parametrize("name", ["four", "five"])
def test_capacity_one_word_short(dev, name):
    """A buffer one word short of the total, for the 4-slot layout (the
    walk-first kernel's checked re-walk) and the 5-payload one (the
    per-window walk): OVERFLOW_PUT at the restatement's record and op,
    nothing written past the capacity, the records before it in place."""
    cp = cp_of(name)
    for n in (16, 65, 257):
        _, nat, heap, full, woffs = batch(name, n)
        cap = full.size - 4
        with pytest.raises(O.OracleError) as oe:
            O.encode(cp, nat, n, heap, cap=cap)
        want = (oe.value.code, oe.value.record, oe.value.op)
        assert want[0] == A.ERR_OVERFLOW_PUT
        for opts in HEAP_OPTS:
            mar = marshaler(dev, name, opts)
            got, offs, err, _ = one_pass(mar, nat, n, heap, cap, dev)
            assert err == want, (name, opts, n)
            a = int(woffs[want[1]])
            assert np.array_equal(got[:a], full[:a]), (name, opts, n)


# ---- round trip through the device's record index
@gpu
@pytest.mark.parametrize("name", ["three", "long9k"])
def test_round_trip_through_the_index(dev, name):
    """Encode, xdrg_index_records over the stream, decode without offsets:
    the index is the constructed offsets, the values come back."""
    t = ZOO[name]
    for n in NS:
        vals, nat, heap, want, woffs = batch(name, n)
        mar = M.Marshaler(M.Plan(t), dev)
        res = mar.encode(to_dev(nat, dev), n, heap_dev(heap, dev))
        assert np.array_equal(res.xdr.cpu().numpy(), want)
        ix = mar.index_records(res.xdr, n)
        assert np.array_equal(ix.cpu().numpy().view(np.uint64), woffs), (name, n)
        back, bheap = mar.decode(res.xdr, n)
        assert OB.unstage(t, back.cpu().numpy(), bheap.cpu().numpy(), n) == vals
