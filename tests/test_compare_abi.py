"""xdrg_plan_set_compare_classes / xdrg_compare without a GPU: argument
checks that return before any HIP call, the class side table leaving the
plan ops untouched, and the compiled kernels' private-segment size."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from xdrpp_amd import _abi as A
from xdrpp_amd import build as B
from xdrpp_amd import schemas as S
from xdrpp_amd import xdr_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(t, classes=True):
    cp = T.compile_plan(t)
    h = C.c_void_p()
    tab = cp.table
    A.check(A.lib().xdrg_plan_create(cp.ops.ctypes.data_as(C.POINTER(A.XdrgOp)), len(cp.ops),
                                     tab.ctypes.data_as(C.POINTER(C.c_uint32)) if tab.size else None, tab.size,
                                     cp.stride, C.byref(h)), "xdrg_plan_create")
    if classes:
        assert _set(h, cp.cmp_classes) == A.OK
    return cp, h


def _set(h, cls, nops=None):
    cls = np.ascontiguousarray(cls, dtype=np.uint8)
    return A.lib().xdrg_plan_set_compare_classes(h, cls.ctypes.data_as(C.c_void_p), len(cls) if nops is None else nops)


def test_set_classes_argument_checks():
    L = A.lib()
    cp, h = _plan(S.rpc_msg, classes=False)
    try:
        good = cp.cmp_classes
        assert L.xdrg_plan_set_compare_classes(None, good.ctypes.data_as(C.c_void_p), len(good)) == -1
        assert L.xdrg_plan_set_compare_classes(h, None, len(good)) == -1
        assert _set(h, good, len(good) - 1) == -1     # wrong nops
        assert _set(h, np.append(good, 0)) == -1
        bad = good.copy()
        bad[0] = 3                                   # U32 op: bool is a discriminant's class only
        assert cp.ops[0]["kind"] == A.OP_U32 and _set(h, bad) == -1
        bad = good.copy()
        bad[1] = 4                                   # UNION op: out of range
        assert cp.ops[1]["kind"] == A.OP_UNION and _set(h, bad) == -1
        ok = good.copy()
        ok[1] = A.CMP_CLASS_BOOL
        assert _set(h, ok) == A.OK and _set(h, good) == A.OK
    finally:
        L.xdrg_plan_destroy(h)


def test_compare_argument_checks_before_any_hip_call():
    L = A.lib()
    cp, h = _plan(S.rec128)
    cv, hv = _plan(S.recvar)
    try:
        a, out = 0x10000, 0x20000  # never dereferenced: every call below returns from the host checks
        assert L.xdrg_compare(None, a, None, 0, a, None, 0, 1, out, None) == -1
        assert L.xdrg_compare(h, None, None, 0, a, None, 0, 1, out, None) == -1
        assert L.xdrg_compare(h, a, None, 0, None, None, 0, 1, out, None) == -1
        assert L.xdrg_compare(h, a, None, 0, a, None, 0, 1, None, None) == -1
        assert L.xdrg_compare(hv, a, None, 16, a, None, 0, 1, out, None) == -1    # a length without a heap
        assert L.xdrg_compare(h, a + 2, None, 0, a, None, 0, 1, out, None) == -2   # fixed: 4-byte records
        assert L.xdrg_compare(h, a, None, 0, a + 1, None, 0, 1, out, None) == -2
        assert L.xdrg_compare(hv, a + 4, None, 0, a, None, 0, 1, out, None) == -2  # var: 8-byte records
        assert L.xdrg_compare(hv, a, a + 2, 16, a, None, 0, 1, out, None) == -2    # 4-byte heaps
        assert L.xdrg_compare(hv, a, a, 16, a, a + 1, 16, 1, out, None) == -2
        assert L.xdrg_compare(h, None, None, 0, None, None, 0, 0, None, None) == A.OK  # n = 0 launches nothing
        assert L.xdrg_compare(hv, a, a, 16, a, a, 16, 0, out, None) == A.OK
    finally:
        L.xdrg_plan_destroy(h)
        L.xdrg_plan_destroy(hv)


@pytest.mark.parametrize("name", ["rec128", "recvar", "rpc"])
def test_plan_without_classes_is_unsupported(name):
    L = A.lib()
    cp, h = _plan(S.ALL[name], classes=False)
    try:
        assert L.xdrg_compare(h, 0x10000, None, 0, 0x10000, None, 0, 1, 0x20000, None) == -3
        assert _set(h, cp.cmp_classes) == A.OK
    finally:
        L.xdrg_plan_destroy(h)


def test_classes_are_a_side_table(monkeypatch):
    """The xdrg_op arrays (and tables) of every schema are what compile_plan
    gave before it knew classes: rebuilt with the class argument ignored."""
    plans = {**S.ALL, **S.CONTAINERS}
    with_cls = {k: T.compile_plan(t) for k, t in plans.items()}
    emit = T._Ctx.emit

    def emit_without(self, *args, cls=0, **kw):
        return emit(self, *args, **kw)

    monkeypatch.setattr(T._Ctx, "emit", emit_without)
    for k, t in plans.items():
        old = T.compile_plan(t)
        assert not old.cmp_classes.any()
        assert old.ops.tobytes() == with_cls[k].ops.tobytes(), k
        assert old.table.tobytes() == with_cls[k].table.tobytes(), k
        assert with_cls[k].cmp_classes.shape == (len(old.ops),) and with_cls[k].cmp_classes.dtype == np.uint8


def test_classes_of_the_scalar_types():
    t = T.Struct("t", [("a", T.Int), ("b", T.UInt), ("c", T.Float), ("d", T.Hyper), ("e", T.UHyper), ("f", T.Double),
                       ("g", T.Bool), ("h", S.other_color),
                       ("u", T.Union("u", "d", T.UInt, [([1], "x", T.Int)])),
                       ("v", T.Union("v", "d", T.Bool, [([1], "x", T.Int)])),
                       ("w", T.Union("w", "d", S.other_color, [([1], "x", T.Float)]))])
    cp = T.compile_plan(t)
    kinds = [int(k) for k in cp.ops["kind"]]
    want = [1, 0, 2, 1, 0, 2, 0, 0, 0, 1, 0, 3, 1, 0, 1, 2, 0, 0]
    assert kinds[:8] == [A.OP_U32] * 3 + [A.OP_U64] * 3 + [A.OP_BOOL, A.OP_ENUM]
    assert cp.cmp_classes.tolist() == want


def test_kernels_use_no_scratch(tmp_path):
    """A hipGraph replayed more than once faulted while frame walks kept
    their frames in private memory (sub_kernels.h); both compare kernels
    must report a private segment of 0 bytes."""
    hipcc = B.hipcc()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    src = tmp_path / "compare_copy.hip"
    shutil.copy(os.path.join(B.CSRC, "compare.hip"), src)
    r = subprocess.run([hipcc, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "--offload-device-only", "-c",
                        "-I", B.CSRC, "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "compare_copy.o"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    fixed = [v for k, v in seen.items() if "k_cmp_fixed" in k]
    walk = [v for k, v in seen.items() if "k_cmp_walk" in k]
    assert len(fixed) == 2 and len(walk) == 2, seen
    assert fixed == [0, 0] and walk == [0, 0], seen
