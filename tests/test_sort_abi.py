"""xdrg_sort_workspace_size / xdrg_sort without a GPU: the argument checks
that return before any HIP call, the workspace size, and the compiled
kernels' private-segment size."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from xdrpp_amd import _abi as A
from xdrpp_amd import build as B
from xdrpp_amd import schemas as S
from xdrpp_amd import xdr_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3


def _plan(t, classes=True):
    cp = T.compile_plan(t)
    h = C.c_void_p()
    tab = cp.table
    A.check(A.lib().xdrg_plan_create(cp.ops.ctypes.data_as(C.POINTER(A.XdrgOp)), len(cp.ops),
                                     tab.ctypes.data_as(C.POINTER(C.c_uint32)) if tab.size else None, tab.size,
                                     cp.stride, C.byref(h)), "xdrg_plan_create")
    if classes:
        cls = cp.cmp_classes
        assert A.lib().xdrg_plan_set_compare_classes(h, cls.ctypes.data_as(C.c_void_p), len(cls)) == A.OK
    return cp, h


def test_sort_argument_checks_before_any_hip_call():
    L = A.lib()
    _, h = _plan(S.rec128)
    _, hv = _plan(S.recvar)
    try:
        # never dereferenced: every call below returns from the host checks
        r, perm, first, cnt, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        big = 1 << 40
        assert L.xdrg_sort(None, r, None, 0, 1, perm, first, cnt, ws, big, None) == EINVAL
        assert L.xdrg_sort(h, None, None, 0, 1, perm, first, cnt, ws, big, None) == EINVAL
        assert L.xdrg_sort(h, r, None, 0, 1, None, first, cnt, ws, big, None) == EINVAL
        assert L.xdrg_sort(h, r, None, 0, 1, perm, first, None, ws, big, None) == EINVAL
        assert L.xdrg_sort(h, r, None, 0, 1, perm, first, cnt, None, big, None) == EINVAL
        assert L.xdrg_sort(hv, r, None, 16, 1, perm, first, cnt, ws, big, None) == EINVAL   # a length without a heap
        for n in (1, 257, 100000):
            need = L.xdrg_sort_workspace_size(h, n)
            assert L.xdrg_sort(h, r, None, 0, n, perm, first, cnt, ws, need - 1, None) == EINVAL
        assert L.xdrg_sort(h, r + 2, None, 0, 1, perm, first, cnt, ws, big, None) == EALIGN   # fixed: 4-byte records
        assert L.xdrg_sort(hv, r + 4, None, 0, 1, perm, first, cnt, ws, big, None) == EALIGN  # var: 8-byte records
        assert L.xdrg_sort(hv, r, r + 2, 16, 1, perm, first, cnt, ws, big, None) == EALIGN    # 4-byte heaps
        assert L.xdrg_sort(h, r, None, 0, 1, perm, first, cnt, ws + 8, big, None) == EALIGN   # 16-byte workspace
        assert L.xdrg_sort(h, r, None, 0, (1 << 31) + 1, perm, first, cnt, ws, big, None) == EUNSUPPORTED
        # n = 0 launches nothing and needs nothing
        assert L.xdrg_sort(h, None, None, 0, 0, None, None, None, None, 0, None) == A.OK
        assert L.xdrg_sort(hv, r, r, 16, 0, perm, first, cnt, ws, 0, None) == A.OK
    finally:
        L.xdrg_plan_destroy(h)
        L.xdrg_plan_destroy(hv)


@pytest.mark.parametrize("name", ["rec128", "recvar", "rpc"])
def test_plan_without_classes_is_unsupported(name):
    L = A.lib()
    _, h = _plan(S.ALL[name], classes=False)
    try:
        assert L.xdrg_sort(h, 0x10000, None, 0, 1, 0x20000, None, 0x40000, 0x50000, 1 << 40, None) == EUNSUPPORTED
    finally:
        L.xdrg_plan_destroy(h)


def test_workspace_size():
    L = A.lib()
    _, h = _plan(S.recvar)
    try:
        sizes = [L.xdrg_sort_workspace_size(h, n) for n in (0, 1, 2, 255, 256, 257, 1000, 1 << 20, 1 << 31)]
        assert sizes[1] > 0
        assert sizes == sorted(sizes)
        assert sizes[-1] >= 2 * 4 * (1 << 31)  # two permutation buffers at the least
    finally:
        L.xdrg_plan_destroy(h)


def test_kernels_use_no_scratch(tmp_path):
    """Frames in private memory made a replayed hipGraph fault
    (sub_kernels.h): every sort kernel must report a private segment of 0
    bytes, as the compare kernels do."""
    hipcc = B.hipcc()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    src = tmp_path / "sort_copy.hip"
    shutil.copy(os.path.join(B.CSRC, "sort.hip"), src)
    r = subprocess.run([hipcc, f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "--offload-device-only", "-c",
                        "-I", B.CSRC, "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
                        "-o", str(tmp_path / "sort_copy.o"), str(src)], capture_output=True, text=True)
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
    sort = {k: v for k, v in seen.items() if "k_sort_" in k}
    for kernel, count in (("k_sort_classify", 2), ("k_sort_emit", 1), ("k_sort_tile", 2), ("k_sort_merge", 2),
                          ("k_sort_first", 2)):
        assert sum(kernel in k for k in sort) == count, seen
    assert not any(sort.values()), sort
    assert not any(v for k, v in seen.items() if "k_tile_scan" in k), seen
