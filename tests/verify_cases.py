"""TEST INFRASTRUCTURE for tests/test_gpu_verify_variants.py: the launch
geometry of the verdict kernels restated from the headers, plans on both sides
of its LDS limit with hand-written records and damage whose answer is known,
and full 64-entry plan tables with their call and reply streams.  Nothing
here needs a GPU: every expected value is the restatement's
(verdict_model.oracle_verdict, reply_model) or a committed fixture's."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from conftest import ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
from xdrpp_amd import workloads as W
from xdrpp_amd.xdr_types import (Bool, Enum, Hyper, Int, Opaque, OpaqueArray, Pointer, String, Struct, UInt, Union,
                                 Void, XArray, XVector, _Scalar, _VarBytes, compile_plan)
import oracle_bridge as O
import reply_batches as RB
import reply_model as RM
import verdict_model as V
import test_fixed_layouts as FL
import test_sub_layouts as SL
import test_var_layouts as VL
from test_deep import big_node_chains

CSRC = os.path.join(ROOT, "xdrpp_amd", "csrc")
OP_BYTES = 32  # sizeof(xdrg_op)
SLACK = 8      # zero bytes after the last record: a span end moved by +4 stays inside the stream


# ------------------------------------------------------------ the geometry
@functools.lru_cache(maxsize=None)
def header_constants():
    """(LDS bytes a workgroup asks for, threads of a SUB workgroup, frames a
    lane) as verify_host.h and verify_kernels.h spell them."""
    host = open(os.path.join(CSRC, "verify_host.h")).read()
    kern = open(os.path.join(CSRC, "verify_kernels.h")).read()
    m = re.search(r"ops_bytes \+ frames <= \((\d+)u << (\d+)\)", host)
    assert m, "verify_geometry's LDS limit"
    t = re.search(r"constexpr uint32_t kVerifySubThreads = (\d+);", kern)
    f = re.search(r"constexpr uint32_t kVerifyFrames = (\w+);", kern)
    w = re.search(r"verify_frame_words\(uint32_t nthreads\) \{ return (\d+)u \* kVerifyFrames \* nthreads; \}", kern)
    assert t and f and w and f.group(1) == "XDRG_INDEX_FRAMES" and int(w.group(1)) == 3
    pub = open(os.path.join(ROOT, "include", "xdrgpu.h")).read()
    frames = int(re.search(r"#define XDRG_INDEX_FRAMES (\d+)", pub).group(1))
    assert frames == A.INDEX_FRAMES
    return int(m.group(1)) << int(m.group(2)), int(t.group(1)), frames


def has_sub(cp) -> bool:
    """plan.cpp's has_sub: a container whose elements are a subroutine."""
    return bool(np.any((cp.ops["kind"] == A.OP_VECTOR) & (cp.ops["flags"] & A.F_SUB != 0)))


def geometry(sub: bool, nops: int):
    """verify_geometry (verify_host.h), restated: (SUB, LDSOPS) of a launch
    over plans that hold `nops` ops together, `sub` if any has element
    subroutines."""
    lds, threads, frames = header_constants()
    fr = 4 * 3 * frames * threads if sub else 0
    return bool(sub), OP_BYTES * nops + fr <= lds


def ops_limit(sub: bool) -> int:
    """The most ops a launch stages in LDS."""
    n = 0
    while geometry(sub, n + 1)[1]:
        n += 1
    return n


# ---------------------------------------------------------- a wire writer
def _be(v: int) -> bytes:
    return (int(v) & 0xFFFFFFFF).to_bytes(4, "big")


def put(t, v, out: bytearray, marks: dict, path: str = "") -> None:
    """The XDR of value `v` of type `t` appended to `out`; marks[path] = where
    each field starts (values as objects.stage takes them)."""
    marks[path] = len(out)
    if t is Bool:
        out += _be(1 if v else 0)
    elif isinstance(t, _Scalar):
        out += (int(v) & ((1 << (8 * t.size)) - 1)).to_bytes(t.size, "big")
    elif isinstance(t, Enum):
        out += _be(v)
    elif isinstance(t, OpaqueArray):
        assert len(v) == t.n
        out += v + bytes(-t.n % 4)
    elif isinstance(t, _VarBytes):
        out += _be(len(v)) + v + bytes(-len(v) % 4)
    elif isinstance(t, XArray):
        for i, e in enumerate(v):
            put(t.elem, e, out, marks, f"{path}[{i}]")
    elif isinstance(t, XVector):
        items = ([] if v is None else [v]) if isinstance(t, Pointer) else list(v)
        out += _be(len(items))
        for i, e in enumerate(items):
            put(t.elem, e, out, marks, f"{path}[{i}]")
    elif isinstance(t, Struct):
        for f, ft in t.fields:
            put(ft, v[f], out, marks, f"{path}.{f}" if path else f)
    elif isinstance(t, Union):
        disc, val = v
        out += _be(disc)
        for cases, f, at in t.arms:
            if disc in cases and at is not Void:
                put(at, val, out, marks, f"{path}.{f}")
    else:
        raise TypeError(t)


# ------------------------------------------- plans around the LDS limit
wtag = Enum("wtag", {"WNEG": -7, "WONE": 1, "WBIG": 1000}, validate=True)
WTAGS = (-7, 1, 1000)
wun = Union("wun", "k", Int, [([0], "", Void), ([1], "i", Int), ([2], "h", Hyper)])
celem = Struct("celem", [("e", wtag), ("o", OpaqueArray(3))])
phyper = Pointer(Hyper)
# every kind verify_walk switches on, with the ops each takes
CYCLE = [(Int, 1), (Hyper, 1), (Bool, 1), (OpaqueArray(5), 1), (Opaque(5), 1), (String(7), 1), (wtag, 1),
         (wun, 5), (phyper, 2)]
litem = Struct("litem", [("s", String(5)), ("fx", OpaqueArray(5)), ("e", wtag), ("u", wun), ("i", Int)])
LITEM_OPS = 10  # its subroutine: five fields, the union's two arms and jumps, END


class LimitPlan:
    """One plan of the limit tests: its type, compiled plan, the op of every
    top-level field, clean records and the damage that suits it."""

    def __init__(self, name, t, family, nops):
        self.name, self.t, self.family, self.nops = name, t, family, nops
        self.cp = compile_plan(t)
        self.sub = has_sub(self.cp)
        self._recs = {}

    # -- values
    def value(self, r, **kw):
        return {"flat": self._flat_value, "big": self._node_value, "frame": self._node_value}[self.family](r, 0, **kw)

    def _flat_value(self, r, _, cv=None, ev=None):
        v = {}
        for j, (f, ft) in enumerate(self.t.fields):
            k = r + j
            forced = (j // len(CYCLE)) % 2 == 0  # lengths that leave pad bytes, in every second cycle
            if f == "pv":
                v[f] = [(k * 0x9E3779B97F4A7C15 + i) & (2 ** 63 - 1) for i in range(r % 5)]
            elif f == "ev":
                v[f] = [WTAGS[(k + i) % 3] for i in range((r + 1) % 4 if ev is None else ev)]
            elif f == "cv":
                v[f] = [{"e": WTAGS[(k + i) % 3], "o": bytes([i + 1, r & 0xFF, 0x80 | i])}
                        for i in range(r % 4 if cv is None else cv)]
            elif ft is Bool:
                v[f] = bool(k & 1)
            elif isinstance(ft, _Scalar):
                v[f] = (r * 7919 + j * 104729) % (2 ** 31 - 1) * (0x100000001 if ft.size == 8 else 1)
            elif ft is wtag:
                v[f] = WTAGS[k % 3]
            elif isinstance(ft, OpaqueArray):
                v[f] = bytes((k + i) & 0xFF | 1 for i in range(ft.n))
            elif isinstance(ft, _VarBytes):
                n = ft.max_len if forced else k % (ft.max_len + 1)
                v[f] = bytes(0x41 + (k + i) % 26 for i in range(n))
            elif ft is wun:
                v[f] = (k % 3, [None, k, k << 33][k % 3])
            elif ft is phyper:
                v[f] = k if forced or k & 1 else None
            else:
                raise TypeError(ft)
        return v

    def _node_value(self, r, i, nodes=None, items=None, name=None):
        nodes = 1 + r % 3 if nodes is None else nodes
        v = {}
        for j, (f, ft) in enumerate(self.t.fields):
            if f == "name":
                v[f] = b"n" * ((r + i) % 11 if name is None else name)
            elif f == "items":
                v[f] = [{"s": bytes(0x61 + (r + q) % 26 for _ in range(5 if q == 0 else (r + q) % 6)),
                         "fx": bytes([q + 1, 2, 3, 4, 0x80 | r & 0x7F]), "e": WTAGS[(r + q) % 3],
                         "u": ((r + q) % 3, [None, q, r << 33][(r + q) % 3]), "i": r * 31 + q}
                        for q in range((r + i) % 4 if items is None else items)]
            elif f == "next":
                v[f] = self._node_value(r, i + 1, nodes, items, name) if i + 1 < nodes else None
            else:
                v[f] = (r * 7919 + i * 104729 + j) & 0xFFFFFFFF
        return v

    def record(self, r, **kw):
        """(bytes, marks) of record r, written by hand."""
        key = (r, tuple(sorted(kw.items())))
        if key not in self._recs:
            out, marks = bytearray(), {}
            put(self.t, self.value(r, **kw), out, marks)
            self._recs[key] = (bytes(out), marks)
        return self._recs[key]

    # -- damage: (kind, field or amount, value overrides the record needs)
    def fields_of(self, kind):
        """Top-level fields of a type, in op order."""
        return [f for f, ft in self.t.fields if ft is kind or (isinstance(kind, type) and type(ft) is kind)]

    def damages(self):
        if self.family == "flat":
            return self._flat_damages()
        return self._node_damages()

    @staticmethod
    def _spread(fs):
        """The first, a middle and the last of a list of fields."""
        return [fs[0], fs[len(fs) // 2], fs[-1]]

    def _forced(self, fs):
        idx = {f: j for j, (f, _) in enumerate(self.t.fields)}
        return [f for f in fs if (idx[f] // len(CYCLE)) % 2 == 0]

    def _flat_damages(self):
        strs, opqs = self._forced(self.fields_of(String)), self._forced(self.fields_of(Opaque))
        fixed, ptrs = self.fields_of(OpaqueArray), self._forced(self.fields_of(Pointer))
        enums, unions, ints = self.fields_of(wtag), self.fields_of(wun), self.fields_of(Int)
        d = [("enum", "first", {})]                                       # the first op
        d += [("len_ff", f, {}) for f in self._spread(strs)]              # OVERFLOW_GET
        d += [("bound", strs[-1], {})]                                    # XSTRING_BOUND
        d += [("bound", opqs[0], {}), ("bound", opqs[-1], {})]            # XVECTOR_BOUND
        d += [("ptr2", ptrs[len(ptrs) // 2], {}), ("ptr2", ptrs[-1], {})]  # POINTER_BOUND
        d += [("pad_fixed", fixed[0], {}), ("pad_fixed", fixed[-1], {})]
        d += [("pad_var", f, {}) for f in self._spread(opqs)]
        d += [("enum", enums[len(enums) // 2], {}), ("enum", enums[-1], {})]
        d += [("disc", unions[0], {}), ("disc", unions[-1], {})]
        d += [("cut", ints[len(ints) // 2], {}), ("cut", ints[-2], {})]   # OVERFLOW_GET at a chosen op
        d += [("end", -4, {}), ("end", 4, {}), ("end", -1, {}), ("end", -2, {}), ("end", -3, {})]
        # the inline vectors: a count one past the bytes left; a bad enum and a pad byte in elements k > 0
        # (and, for comparison, a bad enum in element 0)
        d += [("pv_past", "pv", {}), ("cv_enum", "cv[2].e", {"cv": 3}), ("cv_pad", "cv[1].o", {"cv": 3}),
              ("ev_enum", "ev[2]", {"ev": 4}), ("ev_enum0", "ev[0]", {"ev": 4})]
        return d

    def _node_damages(self):
        two = {"nodes": 2, "name": 5}
        d = [("empty", None, {}), ("len_ff", "name", {}), ("len_ff", "next[0].name", two),
             ("ptr2", "next", {}), ("ptr2", "next[0].next", two), ("pad_var", "name", {"name": 6}),
             ("pad_var", "next[0].name", two), ("cut", "f7", {}), ("cut", f"f{len(self.t.fields) // 2}", {}),
             ("cut", f"next[0].f{len(self.t.fields) - 9}", two),
             ("end", -4, {}), ("end", 4, {}), ("end", -1, {}), ("end", -2, {}), ("end", -3, {})]
        if self.family == "frame":
            it = {"nodes": 2, "items": 3}
            d += [("vec_bound", "items", it), ("vec_bound", "next[0].items", it),
                  ("bound", "items[0].s", it), ("bound", "next[0].items[2].s", it),
                  ("pad_var", "items[0].s", it), ("pad_fixed", "items[1].fx", it),
                  ("pad_fixed", "next[0].items[2].fx", it), ("enum", "items[2].e", it),
                  ("enum", "next[0].items[0].e", it), ("disc", "items[1].u", it),
                  ("disc", "next[0].items[2].u", it), ("len_ff", "items[2].s", it),
                  ("cut", "next[0].items[1].i", it), ("vec_past", "next[0].items", it)]
        return d

    def leaf_type(self, path):
        t = self.t
        for part in re.findall(r"[A-Za-z_]\w*|\[\d+\]", path):
            if part[0] == "[":
                t = t.elem
            elif isinstance(t, Union):
                t = t.arm_by_name(part)
            else:
                t = dict(t.fields)[part]
        return t

    def damaged(self, r, dmg):
        """(bytes, span end relative to the record's start) of record r under
        damage `dmg`; the bytes keep their length (a moved end reads on into
        the next record, or stops short)."""
        kind, f, kw = dmg
        rec, marks = self.record(r, **kw)
        x = bytearray(rec)
        end = len(x)
        if kind == "end":
            return bytes(x), end + f
        if kind == "empty":
            return bytes(x), 0
        at = marks[f]
        t = self.leaf_type(f)
        if kind == "cut":
            end = at
        elif kind == "len_ff":
            x[at:at + 4] = _be(0xFFFFFFFF)
        elif kind in ("bound", "vec_bound"):
            x[at:at + 4] = _be(t.max_len + 1)
        elif kind == "ptr2":
            x[at:at + 4] = _be(2)
        elif kind == "pad_fixed":
            assert t.n % 4
            x[at + t.n] = 0x5A
        elif kind == "pad_var":
            n = int.from_bytes(x[at:at + 4], "big")
            assert n % 4
            x[at + 4 + n + (3 - n % 4)] = 1  # the last pad byte
        elif kind in ("enum", "cv_enum", "ev_enum", "ev_enum0"):
            x[at:at + 4] = _be(5)
        elif kind == "cv_pad":
            x[at + 3] = 0x80
        elif kind == "disc":
            x[at:at + 4] = _be(9)
        elif kind == "pv_past":  # a count one past the bytes left
            x[at:at + 4] = _be((len(x) - at - 4) // 8 + 1)
        elif kind == "vec_past":  # a count whose least bytes pass the bytes left
            x[at:at + 4] = _be(4)
            end = at + 4 + 16
        else:
            raise ValueError(kind)
        return bytes(x), end

    def bool2(self, r):
        """Record r with a bool word of 2 (accepted: any non-zero bool is
        true), or the record itself for a plan without bools."""
        rec, marks = self.record(r)
        bools = self.fields_of(Bool) if self.family == "flat" else []
        if not bools:
            return rec
        x = bytearray(rec)
        at = marks[bools[(r // 2) % len(bools)]]
        x[at:at + 4] = _be(2)
        return bytes(x)


def flat_type(nops: int) -> Struct:
    """A struct of exactly `nops` ops without element subroutines: a
    validated enum first, fields cycling through CYCLE, then an inline vector
    of plain elements (hypers), two of checked elements (a validated enum; a
    struct of a validated enum and an opaque[3]), and a last int."""
    fields = [("first", wtag)]
    budget = nops - 1 - 1 - 2 - 2 - 3 - 1  # END, first, pv, ev, cv, z
    i = 0
    while budget:
        t, cost = CYCLE[i % len(CYCLE)]
        if cost > budget:
            t, cost = Int, 1
        fields.append((f"f{len(fields)}", t))
        budget -= cost
        i += 1
    fields += [("pv", XVector(Hyper)), ("ev", XVector(wtag, 6)), ("cv", XVector(celem, 6)), ("z", Int)]
    return Struct(f"flat{nops}", fields)


def frame_type(nops: int) -> Struct:
    """bignode with a vector of litem elements before `next`: the vector is
    no tail, so every element list opens a frame."""
    k = nops - 4 - LITEM_OPS
    t = Struct(f"frame{nops}")
    t.define([(f"f{i}", UInt) for i in range(k)] + [("name", String()), ("items", XVector(litem, 4)),
                                                  ("next", Pointer(t))])
    return t


# name -> (family, ops).  The limits are 1536 and 768 ops; "past": far enough
# over the limit that ops fail which a staged copy could not hold.
LIMIT_PLANS = {"flat1536": ("flat", 1536), "flat1537": ("flat", 1537), "flat1601": ("flat", 1601),
               "big768": ("big", 768), "big769": ("big", 769),
               "frame768": ("frame", 768), "frame769": ("frame", 769), "frame833": ("frame", 833)}
PAST = {"flat1601": 1536, "frame833": 768}  # plan -> an op index some failure must reach
NS = (1, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def limit_plan(name) -> LimitPlan:
    family, nops = LIMIT_PLANS[name]
    if family == "flat":
        t = flat_type(nops)
    elif family == "big":
        t, _, _ = big_node_chains([], nops - 3)
    else:
        t = frame_type(nops)
    return LimitPlan(name, t, family, nops)


class SpanBatch:
    """n records back to back (and SLACK zero bytes), one span each, and the
    restatement's verdict of every span."""

    def __init__(self, cp, parts, ends, kinds, stack_limit=0xFFFFFFFF):
        self.n = len(parts)
        starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        self.x = np.frombuffer(b"".join(parts) + bytes(SLACK), dtype=np.uint8).copy()
        self.offsets = starts
        self.spans = np.stack([starts[:-1], starts[:-1] + np.asarray(ends, dtype=np.int64)], axis=1)
        self.kinds = kinds  # the damage of each record, None for an intact one
        self.stack_limit = stack_limit
        self.want = V.oracle_verdicts(cp, self.x, self.spans, stack_limit)

    @property
    def bad(self):
        return int(np.count_nonzero(self.want))

    @property
    def share(self):
        return self.bad / self.n

    @property
    def codes(self):
        return {int(v) & 0xFF for v in self.want if v}

    @property
    def ops(self):
        """The op indices of the failing records (record-level ones left out)."""
        return sorted({int(v) >> 8 for v in self.want if v and int(v) >> 8 != V.RECORD_LEVEL})


def damaged_set(n):
    """Records 0, 63, 64 and n - 1 where they exist, and every odd record."""
    return sorted({r for r in (0, 63, 64, n - 1) if r < n} | set(range(1, n, 2)))


@functools.lru_cache(maxsize=None)
def limit_batch(name, n, clean=False) -> SpanBatch:
    """The batch of n records of a limit plan: the records of damaged_set(n)
    take the plan's damages in turn, every other record is intact, every
    fourth of those with a bool word of 2."""
    lp = limit_plan(name)
    dm = lp.damages()
    hit = {} if clean else {r: dm[j % len(dm)] for j, r in enumerate(damaged_set(n))}
    parts, ends, kinds = [], [], []
    for r in range(n):
        if r in hit:
            b, e = lp.damaged(r, hit[r])
        else:
            b = lp.bool2(r) if r % 4 == 2 else lp.record(r)[0]
            e = len(b)
        parts.append(b)
        ends.append(e)
        kinds.append(hit.get(r))
    return SpanBatch(lp.cp, parts, ends, kinds)


def stack_limit_of(name) -> int:
    """One below the depth the plan's deepest records need: the flat plans'
    checked vector elements (struct, vector, struct: 3), a chain's second
    node (struct, pointer, struct: 3)."""
    return 2


@functools.lru_cache(maxsize=None)
def stack_batch(name, n=65) -> SpanBatch:
    """Intact records under stack_limit_of(name): the records without a
    checked element (a second node) decode, the others overflow the stack."""
    lp = limit_plan(name)
    shallow = {} if lp.family == "flat" else {"nodes": 1, "items": 0}
    parts = [lp.record(r, **(shallow if r % 2 == 0 else {}))[0] for r in range(n)]
    return SpanBatch(lp.cp, parts, [len(p) for p in parts], [None] * n, stack_limit_of(name))


# the code every damage kind of the table must draw
DAMAGE_CODES = {A.ERR_OVERFLOW_GET, A.ERR_XVECTOR_BOUND, A.ERR_XSTRING_BOUND, A.ERR_POINTER_BOUND, A.ERR_NONZERO_PAD,
                A.ERR_INVALID_ENUM, A.ERR_BAD_DISCRIMINANT, A.ERR_TRAILING, A.ERR_SIZE_NOT_MULT4}
# bignode has no bounded field, enum or union
BIG_CODES = {A.ERR_OVERFLOW_GET, A.ERR_POINTER_BOUND, A.ERR_NONZERO_PAD, A.ERR_TRAILING, A.ERR_SIZE_NOT_MULT4}


def codes_of(name):
    return BIG_CODES if LIMIT_PLANS[name][0] == "big" else DAMAGE_CODES


# ------------------------------------------------- the fixed and var zoos
EDGES = (0, 63, 64, 256)  # either side of a wave and of a workgroup, and the last record
ZOO_N = 257


@functools.lru_cache(maxsize=None)
def codes_of_what(what: str) -> tuple:
    """The error codes whose xdrg_error_message is a fixture's what()."""
    hits = tuple(c for c in range(1, 21) if A.lib().xdrg_error_message(c).decode() == what)
    assert hits, what
    return hits


class ZooBatch:
    """257 records of a zoo layout, clean, and copies with one damage case in
    the records EDGES: spans, the restatement's verdicts (the clean records'
    computed once, all 0)."""

    def __init__(self, cp, parts):
        self.cp, self.parts = cp, parts
        self.x, self.offsets, self.spans = self.join(parts)
        self.clean = V.oracle_verdicts(cp, self.x, self.spans)
        assert not self.clean.any()

    @staticmethod
    def join(parts):
        offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
        x = np.concatenate(list(parts) + [np.zeros(SLACK, np.uint8)])
        return x, offs, np.stack([offs[:-1], offs[1:]], axis=1)

    def case(self, new_parts: dict, moves: dict | None = None):
        """(stream, offsets, spans, verdicts) with the records of `new_parts`
        replaced and the span ends of `moves` moved."""
        parts = list(self.parts)
        for r, p in new_parts.items():
            parts[r] = p
        x, offs, spans = self.join(parts)
        for r, d in (moves or {}).items():
            spans[r, 1] += d
        want = self.clean.copy()
        for r in set(new_parts) | set(moves or {}):
            want[r] = V.oracle_verdict(self.cp, x, spans[r, 0], spans[r, 1])
        return x, offs, spans, want


@functools.lru_cache(maxsize=None)
def fixed_zoo(name) -> ZooBatch:
    """The fixture's 8 records, then 249 of the module's own (bool words of
    any non-zero value among them)."""
    cp = FL.cp_of(name)
    g = _fixed_gold()[name]
    W_ = cp.fixed_size
    x = np.concatenate([FL.gold_wire(name, g), FL.case(FL.ZOO[name], ZOO_N - 8)[2]])
    return ZooBatch(cp, [x[r * W_:(r + 1) * W_] for r in range(ZOO_N)])


@functools.lru_cache(maxsize=None)
def _fixed_gold():
    import json
    with open(os.path.join(FL.GOLD, "fixed.json")) as f:
        return json.load(f)["structs"]


FIXED_UNDAMAGED = ["id16_bool", "id112", "id208", "lastbool", "bool4", "tailbools", "wide16", "odd7", "vpair", "arr5"]
FIXED_BOOLS = ["id16_bool", "lastbool", "bool4", "tailbools", "wide16", "odd7", "vpair", "arr5"]
MOVES = {0: -4, 63: 4, 64: -2, 256: -4}


def fixed_damaged(name, k):
    """Damage case k of the fixture in the records EDGES."""
    zb = fixed_zoo(name)
    d = _fixed_gold()[name]["damaged"][k]
    new = {}
    for r in EDGES:
        p = zb.parts[r].copy()
        FL.damage(p, 0, dict(d, at_record=0))
        new[r] = p
    return d, zb.case(new)


def fixed_bool2(name):
    """Every bool word of records 1 and 65 set to 2: still verdict 0."""
    zb = fixed_zoo(name)
    new = {}
    for r in (1, 65):
        p = zb.parts[r].copy()
        for _, kind, _, _, woff, _, _ in FL.fields_of(zb.cp):
            if kind == A.OP_BOOL:
                p[woff:woff + 4] = (0, 0, 0, 2)
        new[r] = p
    return zb.case(new)


@functools.lru_cache(maxsize=None)
def var_zoo(name) -> ZooBatch:
    """The fixture's 16 records (twice), then the module's generated ones."""
    _, _, _, x, offs = VL.batch(name, ZOO_N)
    return ZooBatch(VL.cp_of(name), [x[int(offs[r]):int(offs[r + 1])] for r in range(ZOO_N)])


def var_damaged(name, k):
    """Damage case k of the fixture in the records EDGES, each of which
    becomes the fixture's own record of that case, so the damage sits where
    the reference saw it; a resized stream is a moved span end."""
    zb = var_zoo(name)
    d = VL._gold()[name]["damaged"][k]
    w = VL.unhex(d["write"])
    new = {}
    for r in EDGES:
        p = zb.parts[d["at_record"]].copy()
        p[d["offset"]:d["offset"] + w.size] = w
        new[r] = p
    return d, zb.case(new, {r: d["resize"] for r in EDGES} if d["resize"] else None)


@functools.lru_cache(maxsize=None)
def gen_case(seed):
    """257 records of a generated fixed schema, every third span end moved
    by -4, +4 and -2 in turn: (cp, stream, spans, verdicts)."""
    t = FL.gen_schema(seed)
    cp = compile_plan(t)
    x = np.concatenate([FL.case(t, ZOO_N, seed)[2], np.zeros(SLACK, np.uint8)])
    offs = np.arange(ZOO_N + 1, dtype=np.int64) * cp.fixed_size
    spans = np.stack([offs[:-1], offs[1:]], axis=1)
    for j, r in enumerate(range(1, ZOO_N, 3)):
        spans[r, 1] += (-4, 4, -2)[j % 3]
    return cp, x, spans, V.oracle_verdicts(cp, x, spans)


# ------------------------------------------------------ full plan tables
class Entry:
    """One layout of a plan table: its compiled plan, records to draw
    arguments (results) from, and damaged copies."""

    def __init__(self, name, cp, good, bad):
        self.name, self.cp, self._good, self._bad = name, cp, good, bad
        self.sub = has_sub(cp)
        self.nops = len(cp.ops)

    def good(self, i) -> np.ndarray:
        return np.asarray(self._good(i), dtype=np.uint8).copy()

    def bad(self, j) -> np.ndarray:
        return np.asarray(self._bad(j), dtype=np.uint8).copy()


def _resized(p, resize):
    if resize > 0:
        return np.concatenate([p, np.zeros(resize, np.uint8)])
    return p[:resize] if resize < 0 else p


def _fixed_entry(name):
    cp = FL.cp_of(name)
    recs = FL.case(FL.ZOO[name], 32)[2].reshape(32, cp.fixed_size)
    ds = _fixed_gold()[name]["damaged"]

    def bad(j):
        p = recs[j % 32].copy()
        if not ds:
            return _resized(p, (-4, 4)[j % 2])
        FL.damage(p, 0, dict(ds[j % len(ds)], at_record=0))
        return p
    return Entry(name, cp, lambda i: recs[i % 32], bad)


def _var_entry(name):
    cp = VL.cp_of(name)
    _, _, _, x, offs = VL.batch(name, 32)
    parts = [x[int(offs[r]):int(offs[r + 1])] for r in range(32)]
    ds = VL._gold()[name]["damaged"]

    def bad(j):
        d = ds[j % len(ds)]
        p = parts[d["at_record"]].copy()
        w = VL.unhex(d["write"])
        p[d["offset"]:d["offset"] + w.size] = w
        return _resized(p, d["resize"])
    return Entry(name, cp, lambda i: parts[i % 32], bad)


def _sub_entry(name):
    cp = SL.cp_of(name)
    nat, heap = SL.stage(SL.ZOO[name], SL.gold_values(name))
    x, offs = O.encode(cp, nat, 16, heap)
    parts = SL.pieces(x, offs)
    g = SL._gold()[name]["records"]

    def bad(j):
        r = j % 16
        ds = [d for d in g[r]["damaged"] if d[0] != "bool"]
        return SL.damaged_copy(parts[r], ds[(j // 16) % len(ds)])
    return Entry(name, cp, lambda i: parts[i % 16], bad)


def _limit_entry(name):
    lp = limit_plan(name)
    ds = [d for d in lp.damages() if not (d[0] == "end" and d[1] % 4)]  # (a message body is whole words)

    def bad(j):
        b, end = lp.damaged(j, ds[j % len(ds)])
        p = np.frombuffer(b, np.uint8)
        return _resized(p, end - p.size)
    return Entry(name, lp.cp, lambda i: np.frombuffer(lp.record(i % 8)[0], np.uint8), bad)


@functools.lru_cache(maxsize=None)
def entry(name) -> Entry:
    if name in LIMIT_PLANS:
        return _limit_entry(name)
    if name in TABLE_SUBS and name != "mixed":
        return _sub_entry(name)
    return _fixed_entry(name) if name in FL.ZOO else _var_entry(name)


TABLE_BASE = [n for n in FL.ZOO if n not in FL.BIG] + [n for n in VL.ZOO if n != "mixed"]
TABLE_SUBS = ["flatlist", "oddlist", "holder", "listvec", "unode", "vchain", "ping", "mixed"]
SWAP_SLOT = 31
NPLANS = A.RPC_MAX_ARGPLANS


def _table_names(sub: bool, over: bool):
    names = [TABLE_BASE[i % len(TABLE_BASE)] for i in range(NPLANS)]
    if sub:
        for j, slot in enumerate(range(0, NPLANS, 7)):
            names[slot] = TABLE_SUBS[j % len(TABLE_SUBS)]
    if over:
        names[SWAP_SLOT] = "frame833" if sub else "flat1601"
    return names


# table name -> the layouts of its 64 slots
TABLES = {"zoo64": _table_names(False, False), "zoo64_sub": _table_names(True, False),
          "zoo64_over": _table_names(False, True), "zoo64_sub_over": _table_names(True, True)}


def table_geometry(names, void=()):
    """(SUB, LDSOPS) of a launch over a table: the sum over its plans."""
    es = [entry(n) for k, n in enumerate(names) if k not in void]
    return geometry(any(e.sub for e in es), sum(e.nops for e in es))


def slot_key(k):
    """The procedure of table slot k: two programs, so the sort is by more
    than the procedure number."""
    return (200000, 1, k) if k < NPLANS // 2 else (200001, 2, k)


NO_PLAN = (200001, 2, 99)   # registered, no plan
UNREG = (200001, 2, 100)    # not registered
PERIOD = NPLANS + 2         # the call cycle: 66, coprime to 5
DAMAGED = (0, 2)            # a call is damaged when its number mod 5 is one of these
NMSG = 257


def be_words(words):
    return np.array(words, dtype=">u4").view(np.uint8)


class ArgBatch:
    """test_gpu_rpc_args.Batch for a full table: 257 messages whose calls
    cycle through the 64 procedures (then NO_PLAN and UNREG), two calls in
    five damaged, every eighth message no dispatched call; the stream, its
    index and the model of the headers after dispatch + verify_args."""

    def __init__(self, table):
        rng = np.random.default_rng(41)
        self.names = TABLES[table]
        self.keys = [slot_key(k) for k in range(NPLANS)]
        self.entries = {key: entry(n) for key, n in zip(self.keys, self.names)}
        self.cps = {key: e.cp for key, e in self.entries.items()}
        self.procs = R.proc_table({200000: {1: list(range(NPLANS // 2))},
                                   200001: {2: list(range(NPLANS // 2, NPLANS)) + [NO_PLAN[2]]}})
        fs, fo = W.rpc_calls(512)
        fh = O.rpc_headers(fs, fo, W.RPC_PROCS)
        foreign = [fs[int(fo[i]):int(fo[i + 1])] for i in np.nonzero(fh["action"] != A.RPC_DISPATCH)[0]]
        cycle = self.keys + [NO_PLAN, UNREG]
        msgs, ncall, draws, self.damaged_calls = [], 0, {}, []
        for i in range(NMSG):
            if i % 8 == 7:
                msgs.append(foreign[(i // 8) % len(foreign)])
                continue
            key = cycle[ncall % PERIOD]
            e = self.entries.get(key)
            j = draws[key] = draws.get(key, -1) + 1
            if e is None:
                args = be_words(rng.integers(1 << 32, size=int(rng.integers(9))))
            elif ncall % 5 in DAMAGED:
                args = e.bad(ncall // 5)
                self.damaged_calls.append(i)
            else:
                args = e.good(j)
            ncall += 1
            hdr = be_words([int(rng.integers(1 << 32)), 0, 2, key[0], key[1], key[2], 0, 0, 0, 0])
            body = np.concatenate([hdr, args])
            msgs.append(np.concatenate([be_words([body.size | A.MARK_LAST]), body]))
        self.stream = np.concatenate(msgs)
        self.offsets = np.concatenate([[0], np.cumsum([m.size for m in msgs])]).astype(np.uint64)
        self.dispatched = O.rpc_headers(self.stream, self.offsets, self.procs)
        self.model = self.dispatched.copy()
        self.verdicts = np.zeros(NMSG, dtype=np.uint32)
        self.planned = []  # the dispatched calls whose procedure has a plan
        for i, h in enumerate(self.model):
            key = tuple(int(v) for v in h["w"][1:4])
            if h["action"] == A.RPC_DISPATCH and key in self.cps:
                self.planned.append(i)
                v = V.oracle_verdict(self.cps[key], self.stream, h["body_off"], h["end"])
                self.verdicts[i] = v
                if v:
                    self.model[i]["action"] = A.RPC_GARBAGE_ARGS
                    self.model[i]["err"] = v & 0xFF

    def selected(self, key, hdrs=None):
        h = self.model if hdrs is None else hdrs
        return np.nonzero((h["action"] == A.RPC_DISPATCH) & (h["w"][:, 1] == key[0]) &
                          (h["w"][:, 2] == key[1]) & (h["w"][:, 3] == key[2]))[0]

    def slices(self, idx):
        return [self.stream[int(self.model[i]["body_off"]):int(self.model[i]["end"])] for i in idx]


@functools.lru_cache(maxsize=None)
def arg_batch(table) -> ArgBatch:
    return ArgBatch(table)


RES_BASE = 1000                         # result-type numbers start above 0
VOID_SLOTS = tuple(range(0, 63, 9))     # 0, 9, ..., 54: void results between the real ones
NO_PLAN_RES = (2000, 2001)              # result types no verify_results call serves


class ResultBatch:
    """reply_batches.MixedBatch for a full table of result types RES_BASE + k
    (the slots VOID_SLOTS void): 257 messages, success replies whose result
    types cycle through the table, two in five damaged (a void result: 4
    trailing bytes; the last message: a void result with 2), error replies with and without trailing bytes, replies
    to unknown xids, the calls and malformed messages of workloads.rpc_calls;
    300 pending calls, some never answered."""

    NCALLS = 300

    def __init__(self, table):
        rng = np.random.default_rng(43)
        self.names = TABLES[table]
        self.entries = {RES_BASE + k: None if k in VOID_SLOTS else entry(n) for k, n in enumerate(self.names)}
        self.cps = {r: None if e is None else e.cp for r, e in self.entries.items()}
        fs, fo = W.rpc_calls(512)
        fh = O.rpc_headers(fs, fo, None, client=True)
        foreign = [fs[int(fo[i]):int(fo[i + 1])] for i in np.nonzero(
            (fh["action"] == A.RPCR_NOT_REPLY) | (fh["action"] == A.RPCR_MALFORMED))[0]]
        all_x = RB.unique_xids(rng, self.NCALLS + 64)
        self.xids, unknown = all_x[:self.NCALLS], [int(v) for v in all_x[self.NCALLS:]]
        cycle = sorted(self.entries) + list(NO_PLAN_RES)
        self.res = np.array([cycle[c % PERIOD] for c in range(self.NCALLS)], dtype=np.uint32)
        empty = np.zeros(0, dtype=np.uint8)
        msgs, c, nerr, draws = [], 0, 0, {}
        for i in range(NMSG):
            if i % 8 == 7:
                msgs.append(foreign[(i // 8) % len(foreign)])
                continue
            if i % 20 == 9:
                msgs.append(RB.success(unknown.pop(), entry("three").good(i)))
                continue
            if i == NMSG - 1:  # void with 2 trailing bytes: last, since every later message would be misaligned
                self.res[c] = RES_BASE + VOID_SLOTS[1]
                msgs.append(RB.success(int(self.xids[c]), np.zeros(2, np.uint8)))
                c += 1
                continue
            xid, r = int(self.xids[c]), int(self.res[c])
            c += 1
            if (c - 1) % 11 == 6:  # (11: coprime to the cycle, so the error replies move through the table)
                m = RB.error_reply(xid, nerr // 2)
                if nerr % 2:
                    m = RB.message(np.concatenate([m[4:], be_words([int(rng.integers(1 << 32))])]))
                nerr += 1
                msgs.append(m)
                continue
            e = self.entries.get(r)
            j = draws[r] = draws.get(r, -1) + 1
            dmg = (c - 1) % 5 in DAMAGED
            if r not in self.entries:
                result = be_words(rng.integers(1 << 32, size=int(rng.integers(9))))
            elif e is None:  # void: no bytes, or 4 trailing ones
                result = np.zeros(4, np.uint8) if dmg else empty
            else:
                result = e.bad((c - 1) // 5) if dmg else e.good(j)
            msgs.append(RB.success(xid, result))
        self.answered = c
        self.stream, self.offsets = RB.stream_of(msgs)
        self.matched, self.call, self.reply_of = RM.match(self.stream, self.offsets, self.xids)
        self.model = self.matched.copy()
        self.verdicts = RM.verify_results(self.stream, self.model, self.call, self.res, self.cps)
        r_of = np.where(self.call >= 0, self.res[np.clip(self.call, 0, None)], 0)
        # the matched success replies whose result type the table serves
        self.planned = np.nonzero((self.matched["action"] == A.RPCR_OK) & (self.call >= 0) &
                                  (r_of >= RES_BASE) & (r_of < RES_BASE + NPLANS))[0]


def forged_void(b: ResultBatch):
    """The matched headers with the first clean reply of void slot 0 forged to
    end 2 bytes after its body starts, and the model's verdicts of a
    verify_results call that serves that slot alone."""
    res = b.res[np.clip(b.call, 0, None)]
    i = [i for i in b.planned if res[i] == RES_BASE + VOID_SLOTS[0] and not b.verdicts[i]][0]
    h = b.matched.copy()
    h["end"][i] = h["body_off"][i] + 2
    model = h.copy()
    return h, RM.verify_results(b.stream, model, b.call, b.res, {RES_BASE + VOID_SLOTS[0]: None})


@functools.lru_cache(maxsize=None)
def result_batch(table) -> ResultBatch:
    return ResultBatch(table)


# ------------------------------------------------------ the variant table
# (entry point, SUB, LDSOPS) -> what lands there: a limit plan for
# xdrg_verify, a plan table for the RPC kernels.
VARIANTS = {
    ("xdrg_verify", False, True): "flat1536",
    ("xdrg_verify", False, False): "flat1537",
    ("xdrg_verify", True, True): "frame768",
    ("xdrg_verify", True, False): "frame769",
    ("xdrg_rpc_verify_args", False, True): "zoo64",
    ("xdrg_rpc_verify_args", False, False): "zoo64_over",
    ("xdrg_rpc_verify_args", True, True): "zoo64_sub",
    ("xdrg_rpc_verify_args", True, False): "zoo64_sub_over",
    ("xdrg_rpc_verify_results", False, True): "zoo64",
    ("xdrg_rpc_verify_results", False, False): "zoo64_over",
    ("xdrg_rpc_verify_results", True, True): "zoo64_sub",
    ("xdrg_rpc_verify_results", True, False): "zoo64_sub_over",
}


def variant_of(entry_point, what):
    """The (SUB, LDSOPS) the restated geometry gives a plan or table."""
    if entry_point == "xdrg_verify":
        lp = limit_plan(what)
        return geometry(lp.sub, lp.nops)
    return table_geometry(TABLES[what], VOID_SLOTS if entry_point == "xdrg_rpc_verify_results" else ())
