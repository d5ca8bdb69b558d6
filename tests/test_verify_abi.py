"""CPU: the host side of xdrg_verify / xdrg_rpc_verify_args (include/xdrgpu.h
"Per-record decode verdicts"): the xdrg_rpc_argplan layout, and the argument
validation that runs before any HIP call -- so it answers on a machine with
no GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import marshal as M
from xdrpp_amd import schemas as S

EINVAL = -1
FAKE = 0x10000  # a nonzero, 64 KiB-aligned address no call may dereference


LAYOUT_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "xdrgpu.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
#define Z(T) printf(#T " %zu\n", sizeof(T))
int main(void) {
  Z(xdrg_rpc_argplan); F(xdrg_rpc_argplan, prog); F(xdrg_rpc_argplan, vers);
  F(xdrg_rpc_argplan, proc); F(xdrg_rpc_argplan, rsv); F(xdrg_rpc_argplan, plan);
  printf("XDRG_RPC_MAX_ARGPLANS %u\n", XDRG_RPC_MAX_ARGPLANS);
  printf("XDRG_INDEX_FRAMES %u\n", (unsigned)XDRG_INDEX_FRAMES);
  return 0;
}
"""


def test_argplan_layout(tmp_path):
    """xdrg_rpc_argplan as gcc lays it out == its ctypes mirror."""
    src = tmp_path / "probe.c"
    src.write_text(LAYOUT_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert got["xdrg_rpc_argplan"] == C.sizeof(A.XdrgRpcArgplan) == 24
    for f, _ in A.XdrgRpcArgplan._fields_:
        assert got[f"xdrg_rpc_argplan.{f}"] == getattr(A.XdrgRpcArgplan, f).offset, f
    assert got["XDRG_RPC_MAX_ARGPLANS"] == A.RPC_MAX_ARGPLANS
    assert got["XDRG_INDEX_FRAMES"] == A.INDEX_FRAMES


@pytest.fixture(scope="module")
def plan():
    return M.Plan(S.recvar)


def verify(plan_handle, n, stride=8, verdicts=FAKE, begin=FAKE, end=FAKE + 8):
    return A.lib().xdrg_verify(plan_handle, FAKE, 1024, begin, end, stride, n, A.DEFAULT_STACK_LIMIT,
                               verdicts, None, None)


def test_verify_validates_before_any_hip_call(plan):
    assert verify(None, 4) == EINVAL                    # NULL plan
    assert verify(None, 0) == EINVAL                    # ... also with nothing to do
    assert verify(plan.handle, 4, verdicts=None) == EINVAL
    assert verify(plan.handle, 4, begin=None) == EINVAL
    assert verify(plan.handle, 4, end=None) == EINVAL
    for stride in (0, 4, 7, 12, 63):                    # a multiple of 8, at least 8
        assert verify(plan.handle, 4, stride=stride) == EINVAL, stride
        assert verify(plan.handle, 0, stride=stride) == EINVAL, stride


def test_verify_of_nothing_is_ok(plan):
    """n == 0: XDRG_OK, nothing launched (no device is touched here)."""
    for stride in (8, 16, 64):
        assert verify(plan.handle, 0, stride=stride) == A.OK
    assert verify(plan.handle, 0, verdicts=None, begin=None, end=None) == A.OK


def argplans(rows):
    arr = (A.XdrgRpcArgplan * max(len(rows), 1))()
    for i, (prog, vers, proc, handle) in enumerate(rows):
        arr[i] = A.XdrgRpcArgplan(prog, vers, proc, 0, handle)
    return arr


def verify_args(rows, n=4, nplans=None):
    return A.lib().xdrg_rpc_verify_args(FAKE, 1024, FAKE, n, argplans(rows),
                                        len(rows) if nplans is None else nplans,
                                        A.DEFAULT_STACK_LIMIT, None, None)


def test_rpc_verify_args_validates_before_any_hip_call(plan):
    h = plan.handle
    assert verify_args([(1, 1, p, h) for p in range(65)]) == EINVAL       # more than 64 procedures
    assert verify_args([(1, 1, 2, h), (1, 1, 1, h)]) == EINVAL            # unsorted by proc
    assert verify_args([(1, 2, 0, h), (1, 1, 5, h)]) == EINVAL            # ... by vers
    assert verify_args([(2, 0, 0, h), (1, 9, 9, h)]) == EINVAL            # ... by prog
    assert verify_args([(1, 1, 1, h), (1, 1, 1, h)]) == EINVAL            # duplicate
    assert verify_args([(1, 1, 1, h), (1, 1, 2, None)]) == EINVAL         # NULL plan
    assert A.lib().xdrg_rpc_verify_args(FAKE, 1024, FAKE, 4, None, 1, 0, None, None) == EINVAL
    # a valid table and an empty batch: OK, nothing launched
    assert verify_args([(1, 1, p, h) for p in range(64)], n=0) == A.OK
    assert verify_args([(1, 1, 1, h), (1, 2, 0, h), (3, 0, 0, h)], n=0) == A.OK
    assert verify_args([], n=0) == A.OK


def test_python_verify_args_refuses_65_procedures(plan):
    import torch
    from xdrpp_amd import rpc as R
    empty = torch.empty(0, dtype=torch.uint8)
    with pytest.raises(ValueError):
        R.verify_args(empty, empty, {(7, 1, p): plan for p in range(65)})


def test_verdict_error_matches_error_from(plan):
    """verdict_error builds what error_from builds from a status block."""
    assert M.verdict_error(plan, 0, 5) is None
    e = M.verdict_error(plan, (3 << 8) | A.ERR_XSTRING_BOUND, 7)
    assert isinstance(e, M.XdrOverflow) and (e.record, e.op, e.code) == (7, 3, A.ERR_XSTRING_BOUND)
    assert e.what == A.lib().xdrg_error_message(A.ERR_XSTRING_BOUND).decode()
    e = M.verdict_error(plan, (0xFFFF << 8) | A.ERR_TRAILING, 2)
    assert isinstance(e, M.XdrBadMessageSize) and e.op is None and e.record == 2
