"""CPU: the host side of xdrg_rpc_reply_batch (include/xdrgpu.h "Server reply
batch"): the xdrg_rpc_result_src layout read from the header, the argument
validation that runs before any HIP call, the workspace size, the numpy model
of the contract (reply_stream_model.py) against the reference's own bytes,
and the golden batch of test_gpu_reply_batch.py as a test (no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
import reply_stream_model as RS

EINVAL, EALIGN, ESPACE = -1, -2, -6
FAKE = 0x10000  # a nonzero, 64 KiB-aligned address no call may dereference

LAYOUT_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "xdrgpu.h"
#define F(f) printf(#f " %zu\n", offsetof(xdrg_rpc_result_src, f))
int main(void) {
  printf("sizeof %zu\n", sizeof(xdrg_rpc_result_src));
  F(d_bytes); F(d_offsets); F(d_index); F(d_count); F(bytes_len); F(count_cap); F(fixed_size);
  printf("MAX_SRCS %u\n", XDRG_RPC_MAX_RESULT_SRCS);
  printf("ABI %d\n", XDRG_ABI_VERSION);
  return 0;
}
"""


def test_result_src_layout(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(LAYOUT_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["sizeof"] == C.sizeof(A.XdrgRpcResultSrc) == 48
    want = {"d_bytes": 0, "d_offsets": 8, "d_index": 16, "d_count": 24, "bytes_len": 32, "count_cap": 40,
            "fixed_size": 44}
    for f, _ in A.XdrgRpcResultSrc._fields_:
        assert got[f] == getattr(A.XdrgRpcResultSrc, f).offset == want[f], f
    assert got["MAX_SRCS"] == A.RPC_MAX_RESULT_SRCS == 64
    assert got["ABI"] == A.ABI_VERSION == A.lib().xdrg_abi_version() == 10


# ------------------------------------------------------- host validation
def src(d_bytes=FAKE, d_offsets=None, d_index=FAKE, d_count=None, bytes_len=1024, count_cap=8, fixed_size=128):
    return A.XdrgRpcResultSrc(d_bytes, d_offsets, d_index, d_count, bytes_len, count_cap, fixed_size)


def call(n=4, hdrs=FAKE, srcs=(), nsrcs=None, table=True, out=FAKE, cap=4096, offsets=FAKE, unused=None, ws=FAKE,
         ws_bytes=1 << 24, status=FAKE):
    arr = (A.XdrgRpcResultSrc * max(len(srcs), 1))(*srcs) if table else None
    return A.lib().xdrg_rpc_reply_batch(hdrs, n, arr, len(srcs) if nsrcs is None else nsrcs, out, cap, offsets,
                                        unused, ws, ws_bytes, status, None)


def test_reply_batch_validates_before_any_hip_call():
    for n in (4, 0):
        assert call(n=n, offsets=None) == EINVAL
        assert call(n=n, status=None) == EINVAL
        assert call(n=n, nsrcs=1, table=False) == EINVAL           # no table
        assert call(n=n, srcs=[src()] * 65) == EINVAL               # more than 64 sources
        assert call(n=n, srcs=[src(), src(d_index=None)]) == EINVAL  # entries, and nothing that names their messages
        assert call(n=n, srcs=[src(d_bytes=None)]) == EINVAL         # void results with a size
        assert call(n=n, srcs=[src(fixed_size=0)]) == EINVAL         # fixed-size results without one
        assert call(n=n, srcs=[src(fixed_size=126)]) == EINVAL       # ... or one that is not whole words
    assert call(hdrs=None) == EINVAL
    # what is legal: no index for no entries; void results; offsets in place of a size
    assert call(srcs=[src(d_index=None, count_cap=0)], ws_bytes=0) == ESPACE
    assert call(srcs=[src(d_bytes=None, fixed_size=0), src(d_offsets=FAKE, fixed_size=0)], ws_bytes=0) == ESPACE
    assert call(srcs=[src(d_bytes=None, d_offsets=FAKE, fixed_size=0)], ws_bytes=0) == ESPACE
    # alignment: headers 16, u64 arrays 8, bytes 4
    assert call(hdrs=FAKE + 8) == EALIGN
    assert call(offsets=FAKE + 4) == EALIGN
    assert call(unused=FAKE + 4) == EALIGN
    assert call(out=FAKE + 2) == EALIGN
    assert call(srcs=[src(d_bytes=FAKE + 2)]) == EALIGN
    assert call(srcs=[src(d_offsets=FAKE + 4)]) == EALIGN
    assert call(srcs=[src(), src(d_index=FAKE + 4)]) == EALIGN
    assert call(srcs=[src(d_count=FAKE + 4)]) == EALIGN
    # workspace
    need = A.lib().xdrg_rpc_reply_batch_workspace_size(4)
    assert call(ws_bytes=need - 1) == ESPACE and call(ws=None) == ESPACE
    assert call(srcs=[src()] * 64, ws_bytes=need - 1) == ESPACE  # 64 sources pass the validation


def test_workspace_size():
    L = A.lib()
    sizes = [L.xdrg_rpc_reply_batch_workspace_size(n) for n in (1, 256, 257, 1 << 20)]
    assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
    assert sizes == sorted(sizes), sizes
    assert sizes[-1] >= 8 * (1 << 20)  # an owner word per message


def test_python_refuses_more_than_64_sources():
    import torch
    idx = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        R.reply_batch(torch.zeros(64, dtype=torch.uint8), [(idx, None, None)] * 65)


# ----------------------------------- the model against the reference's bytes
def test_model_error_replies_are_the_references():
    hdrs = RS.g("rpccall_1024.hdrs").view(R.HDR_DTYPE)
    stream, offsets, unused, err = RS.model(hdrs, [])
    assert stream.tobytes() == RS.g("rpccall_1024.replies").tobytes()
    assert np.array_equal(offsets, RS.g("rpccall_1024.replyoffs", "<u8"))
    assert unused == 0 and err is None


def success_case():
    """512 DISPATCH headers with the xids of success_rec128_512.msgs and one
    fixed-size source holding each message's result bytes (28..155)."""
    n = 512
    msgs = RS.g("success_rec128_512.msgs")
    assert msgs.size == 156 * n
    hdrs = np.zeros(n, dtype=R.HDR_DTYPE)
    hdrs["action"] = A.RPC_DISPATCH
    hdrs["xid"] = (np.arange(n, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    results = np.ascontiguousarray(msgs.reshape(n, 156)[:, 28:]).reshape(-1)
    return hdrs, RS.Src(np.arange(n, dtype=np.uint64), results, None, 128), msgs


def test_model_success_replies_are_the_references():
    hdrs, source, msgs = success_case()
    stream, offsets, unused, err = RS.model(hdrs, [source])
    assert stream.tobytes() == msgs.tobytes()
    assert np.array_equal(offsets, np.arange(513, dtype=np.uint64) * 156)
    assert unused == 0 and err is None


# ------------------------------------------------- the golden batch is a test
@pytest.fixture(scope="module")
def batch():
    return RS.GoldenBatch()


def test_the_golden_batch_is_a_test(batch):
    assert np.count_nonzero(batch.hdrs["action"] == A.RPC_DISPATCH) == 790 and len(batch.procs) == 61
    counts = [int(np.count_nonzero(batch.kind == k)) for k in range(4)]
    print("calls per class (rec128, recvar, void, unserved):", counts)
    assert all(c >= 150 for c in counts), counts
    assert counts == [201, 213, 176, 200]
    srcs = batch.per_procedure()
    assert len(srcs) == 46
    assert [sum(1 for s in srcs if s.xdr is not None and s.offsets is None),
            sum(1 for s in srcs if s.offsets is not None), sum(1 for s in srcs if s.xdr is None)] == [16, 15, 15]  # ranks 0..60 mod 4
    err = np.isin(batch.hdrs["action"], (A.RPC_RPC_MISMATCH, A.RPC_PROG_UNAVAIL, A.RPC_PROG_MISMATCH,
                                         A.RPC_PROC_UNAVAIL, A.RPC_GARBAGE_ARGS, A.RPC_SYSTEM_ERR, A.RPC_AUTH_ERROR))
    success = np.isin(batch.kind, (RS.REC128, RS.RECVAR, RS.VOID))
    silent = ~err & ~success
    for w0 in range(0, batch.n, 64):  # every wave writes all three
        w = slice(w0, w0 + 64)
        assert success[w].any() and err[w].any() and silent[w].any(), w0


def test_model_equals_the_stream_assembled_from_reference_bytes(batch):
    want, want_offs = batch.expected()
    for srcs in (batch.per_procedure(), batch.per_type()):
        stream, offsets, unused, err = RS.model(batch.hdrs, srcs)
        assert stream.tobytes() == want.tobytes() and np.array_equal(offsets, want_offs)
        assert unused == 0 and err is None
