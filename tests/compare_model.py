"""Python model of xdrg_compare: xdr::operator<=> / operator== (xdrpp/
types.h:946-1062, XDRPP_STRONG_ORDER = 0; pointer's at :647-657) over a
CompiledPlan's ops, its cmp_classes and native + heap arrays.  TEST
INFRASTRUCTURE: the readable statement of the rules the kernels reproduce.

    compare(cp, nat_a, heap_a, nat_b, heap_b, n) -> int8[n] of _abi.CMP_*
"""
from __future__ import annotations

import struct

import numpy as np

from xdrpp_amd import _abi as A

LESS, EQUAL, GREATER, UNORDERED, DEEP, BADREF = (A.CMP_LESS, A.CMP_EQUAL, A.CMP_GREATER, A.CMP_UNORDERED,
                                                 A.CMP_DEEP, A.CMP_BADREF)


class _Stop(Exception):
    def __init__(self, result):
        self.result = result


def _ord(a, b) -> int:
    return LESS if a < b else GREATER if a > b else EQUAL


def _ieee(a: float, b: float) -> int:
    if a != a or b != b:
        return UNORDERED  # a NaN is unordered against everything, itself included
    return _ord(a, b)     # (-0.0 == +0.0)


def _scalar(kind: int, cls: int, a: bytes, b: bytes) -> int:
    if kind == A.OP_BOOL:
        return _ord(a[0] != 0, b[0] != 0)  # any nonzero native byte is true
    if kind == A.OP_ENUM:
        cls = A.CMP_CLASS_SIGNED
    wide = kind == A.OP_U64
    if cls == A.CMP_CLASS_IEEE:
        f = "<d" if wide else "<f"
        return _ieee(struct.unpack(f, a)[0], struct.unpack(f, b)[0])
    signed = cls == A.CMP_CLASS_SIGNED
    return _ord(int.from_bytes(a, "little", signed=signed), int.from_bytes(b, "little", signed=signed))


def _bytes(a: bytes, b: bytes) -> int:
    return _ord(a, b)  # Python orders bytes as unsigned chars, then by length


class _Side:
    def __init__(self, nat: np.ndarray, heap: np.ndarray | None):
        self.nat = nat.tobytes()
        self.heap = b"" if heap is None else heap.tobytes()

    def ref(self, obj: bytes, noff: int):
        off, ln = struct.unpack_from("<QI", obj, noff)
        return off, ln

    def span(self, off: int, nbytes: int) -> bytes:
        if nbytes and (off > len(self.heap) or nbytes > len(self.heap) - off):
            raise _Stop(BADREF)  # outside the heap: nothing is read through it
        return self.heap[off:off + nbytes] if nbytes else b""


def _union_target(cp, op, d: int):
    tab = cp.table
    for i in range(int(op["arg3"])):
        if int(tab[int(op["arg2"]) + 2 * i]) == d:
            return int(tab[int(op["arg2"]) + 2 * i + 1])
    return int(op["arg4"]) if int(op["flags"]) & A.F_DEFAULT else None


def _union_end(cp, u: int) -> int:
    """The pc behind the union at u: where a void arm's case points; every
    other arm ends with a JUMP (at the union's depth) to it."""
    op, ops = cp.ops[u], cp.ops
    tg = [int(cp.table[int(op["arg2"]) + 2 * i + 1]) for i in range(int(op["arg3"]))]
    if int(op["flags"]) & A.F_DEFAULT:
        tg.append(int(op["arg4"]))
    m = max(tg + [u + 1])
    for q in range(u + 1, m):
        if ops[q]["kind"] == A.OP_JUMP and ops[q]["depth"] == op["depth"] and int(ops[q]["arg0"]) == m:
            return m
    for q in range(m, len(ops)):
        e = ops[q]
        if e["kind"] == A.OP_JUMP and e["depth"] == op["depth"]:
            return int(e["arg0"])
        if e["kind"] == A.OP_END or e["depth"] < op["depth"] or (e["kind"] == A.OP_UNION and e["depth"] == op["depth"]):
            break
    return m


def _tail(ops, pc: int) -> bool:
    q = pc + 1
    while ops[q]["kind"] == A.OP_JUMP:
        q = int(ops[q]["arg0"])
    return ops[q]["kind"] == A.OP_END


def _walk(cp, cls, sa: _Side, sb: _Side, oa: bytes, ob: bytes, pc: int, frames: int, last: bool,
          max_frames: int) -> None:
    """Compare the objects oa / ob from pc to the next END; raises _Stop at
    the first field that is not equivalent.  frames = the element frames
    open (a tail container of a last element reuses its frame)."""
    ops = cp.ops
    while True:
        op = ops[pc]
        k, noff = int(op["kind"]), int(op["noff"])
        if k == A.OP_END:
            return
        if k == A.OP_JUMP:
            pc = int(op["arg0"])
            continue
        if k == A.OP_UNION:
            r = _union_disc(int(cls[pc]), oa[noff:noff + 4], ob[noff:noff + 4])
            if r != EQUAL:
                raise _Stop(r)
            t = _union_target(cp, op, int.from_bytes(oa[noff:noff + 4], "little"))
            pc = _union_end(cp, pc) if t is None else t  # no arm: equivalent, on behind the union
            continue
        if k in (A.OP_VAROPAQUE, A.OP_STRING):
            (fa, la), (fb, lb) = sa.ref(oa, noff), sb.ref(ob, noff)
            xa, xb = sa.span(fa, la), sb.span(fb, lb)
            r = _bytes(xa, xb)
        elif k == A.OP_VECTOR:
            (fa, na), (fb, nb) = sa.ref(oa, noff), sb.ref(ob, noff)
            es = int(op["arg1"])
            ea, eb = sa.span(fa, na * es), sb.span(fb, nb * es)
            m = min(na, nb)
            after = _ord(na, nb)  # the shorter container is less; absent < present
            if not int(op["flags"]) & A.F_SUB:
                ne = int(op["arg2"])
                for i in range(m):
                    for j in range(ne):
                        e = ops[pc + 1 + j]
                        r = _field(e, int(cls[pc + 1 + j]), ea[i * es:(i + 1) * es], eb[i * es:(i + 1) * es])
                        if r != EQUAL:
                            raise _Stop(r)
                if after != EQUAL:
                    raise _Stop(after)
                pc += 1 + ne
                continue
            if m:
                tail = frames > 0 and last and _tail(ops, pc)
                inner = frames if tail else frames + 1
                if inner > max_frames:
                    raise _Stop(DEEP)
                for i in range(m):
                    _walk(cp, cls, sa, sb, ea[i * es:(i + 1) * es], eb[i * es:(i + 1) * es], int(op["arg4"]),
                          inner, i == m - 1, max_frames)
            r = after
        else:
            r = _field(op, int(cls[pc]), oa, ob)
        if r != EQUAL:
            raise _Stop(r)
        pc += 1


def _union_disc(c: int, a: bytes, b: bytes) -> int:
    if c == A.CMP_CLASS_BOOL:
        return _ord(a != b"\0\0\0\0", b != b"\0\0\0\0")
    return _scalar(A.OP_U32, c, a, b)


def _field(op, c: int, oa: bytes, ob: bytes) -> int:
    k, noff = int(op["kind"]), int(op["noff"])
    if k == A.OP_OPAQUE:
        n = int(op["arg0"])
        return _bytes(oa[noff:noff + n], ob[noff:noff + n])
    size = {A.OP_U32: 4, A.OP_ENUM: 4, A.OP_U64: 8, A.OP_BOOL: 1}[k]
    return _scalar(k, c, oa[noff:noff + size], ob[noff:noff + size])


def compare(cp, nat_a: np.ndarray, heap_a, nat_b: np.ndarray, heap_b, n: int,
            max_frames: int = A.SUB_FRAMES) -> np.ndarray:
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    sa, sb = _Side(nat_a, heap_a), _Side(nat_b, heap_b)
    out = np.zeros(n, dtype=np.int8)
    st = cp.stride
    for i in range(n):
        try:
            _walk(cp, cp.cmp_classes, sa, sb, sa.nat[i * st:(i + 1) * st], sb.nat[i * st:(i + 1) * st], 0, 0,
                  False, max_frames)
        except _Stop as s:
            out[i] = s.result
    return out
