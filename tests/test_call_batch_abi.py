"""CPU: the host side of the client call batch (include/xdrgpu.h "Client call
batch"): the xdrg_rpc_arg_src layout read from the header, the argument
validation of the three calls that runs before any HIP call, the workspace
size, and the numpy model of the contract (call_stream_model.py) pinned to the
reference: the golden batch's stream through the C restatement of the
server's header decode, through the reference itself, and against what
compile_plan(call_type(T)) marshals.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
from xdrpp_amd import schemas as S
from xdrpp_amd import workloads as W
from xdrpp_amd.xdr_types import compile_plan
import call_stream_model as CS
import oracle_bridge as O

EINVAL, EALIGN, ESPACE = -1, -2, -6
FAKE = 0x10000  # a nonzero, 64 KiB-aligned address no call may dereference

LAYOUT_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "xdrgpu.h"
#define F(f) printf(#f " %zu\n", offsetof(xdrg_rpc_arg_src, f))
int main(void) {
  printf("sizeof %zu\n", sizeof(xdrg_rpc_arg_src));
  F(d_bytes); F(d_offsets); F(d_index); F(d_count); F(bytes_len); F(count_cap); F(fixed_size);
  F(prog); F(vers); F(proc); F(res);
  printf("MAX_SRCS %u\n", XDRG_RPC_MAX_ARG_SRCS);
  printf("UNSENT %u\n", XDRG_RPC_RES_UNSENT);
  printf("ABI %d\n", XDRG_ABI_VERSION);
  return 0;
}
"""


def test_arg_src_layout(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(LAYOUT_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["sizeof"] == C.sizeof(A.XdrgRpcArgSrc) == 64
    want = {"d_bytes": 0, "d_offsets": 8, "d_index": 16, "d_count": 24, "bytes_len": 32, "count_cap": 40,
            "fixed_size": 44, "prog": 48, "vers": 52, "proc": 56, "res": 60}
    assert [f for f, _ in A.XdrgRpcArgSrc._fields_] == list(want)
    for f, _ in A.XdrgRpcArgSrc._fields_:
        assert got[f] == getattr(A.XdrgRpcArgSrc, f).offset == want[f], f
    assert got["MAX_SRCS"] == A.RPC_MAX_ARG_SRCS == 64
    assert got["UNSENT"] == A.RPC_RES_UNSENT == 0xFFFFFFFF
    assert got["ABI"] == A.ABI_VERSION == A.lib().xdrg_abi_version() == 10


# ------------------------------------------------------- host validation
def src(d_bytes=FAKE, d_offsets=None, d_index=FAKE, d_count=None, bytes_len=1024, count_cap=8, fixed_size=128):
    return A.XdrgRpcArgSrc(d_bytes, d_offsets, d_index, d_count, bytes_len, count_cap, fixed_size, 100000, 2, 1, 0)


def call(n=4, xids=FAKE, srcs=(), nsrcs=None, table=True, out=FAKE, cap=4096, offsets=FAKE, sent=None, counts=None,
         ws=FAKE, ws_bytes=1 << 24, status=FAKE):
    arr = (A.XdrgRpcArgSrc * max(len(srcs), 1))(*srcs) if table else None
    return A.lib().xdrg_rpc_call_batch(xids, n, arr, len(srcs) if nsrcs is None else nsrcs, out, cap, offsets,
                                       sent, counts, ws, ws_bytes, status, None)


def test_call_batch_validates_before_any_hip_call():
    for n in (4, 0):
        assert call(n=n, offsets=None) == EINVAL
        assert call(n=n, status=None) == EINVAL
        assert call(n=n, nsrcs=1, table=False) == EINVAL           # no table
        assert call(n=n, srcs=[src()] * 65) == EINVAL               # more than 64 sources
        assert call(n=n, srcs=[src(), src(d_index=None)]) == EINVAL  # entries, and nothing that names their calls
        assert call(n=n, srcs=[src(d_bytes=None)]) == EINVAL         # no arguments, with a size
        assert call(n=n, srcs=[src(fixed_size=0)]) == EINVAL         # fixed-size arguments without one
        assert call(n=n, srcs=[src(fixed_size=126)]) == EINVAL       # ... or one that is not whole words
        assert call(n=n, out=None) == EINVAL                         # a capacity and no output
    assert call(xids=None) == EINVAL
    # what is legal: no index for no entries; no arguments; offsets in place of a size
    assert call(srcs=[src(d_index=None, count_cap=0)], ws_bytes=0) == ESPACE
    assert call(srcs=[src(d_bytes=None, fixed_size=0), src(d_offsets=FAKE, fixed_size=0)], ws_bytes=0) == ESPACE
    assert call(srcs=[src(d_bytes=None, d_offsets=FAKE, fixed_size=0)], ws_bytes=0) == ESPACE
    assert call(out=None, cap=0, ws_bytes=0) == ESPACE
    # alignment: u64 arrays, d_sent and d_counts 8, xids and bytes 4
    assert call(xids=FAKE + 2) == EALIGN
    assert call(offsets=FAKE + 4) == EALIGN
    assert call(sent=FAKE + 4) == EALIGN
    assert call(counts=FAKE + 4) == EALIGN
    assert call(out=FAKE + 2) == EALIGN
    assert call(ws=FAKE + 4) == EALIGN
    assert call(srcs=[src(d_bytes=FAKE + 2)]) == EALIGN
    assert call(srcs=[src(d_offsets=FAKE + 4)]) == EALIGN
    assert call(srcs=[src(), src(d_index=FAKE + 4)]) == EALIGN
    assert call(srcs=[src(d_count=FAKE + 4)]) == EALIGN
    assert call(xids=FAKE + 4, sent=FAKE + 8, counts=FAKE + 16, ws_bytes=0) == ESPACE  # aligned enough
    # workspace
    need = A.lib().xdrg_rpc_call_batch_workspace_size(4)
    assert call(ws_bytes=need - 1) == ESPACE and call(ws=None) == ESPACE
    assert call(srcs=[src()] * 64, ws_bytes=need - 1) == ESPACE  # 64 sources pass the validation


def test_next_xids_validates_before_any_hip_call():
    f = A.lib().xdrg_rpc_next_xids
    assert f(FAKE, 0xFFFFFFFF, 0, 1, FAKE, None) == EINVAL          # no free value is left
    assert f(FAKE, 1, 0, 0xFFFFFFFF, FAKE, None) == EINVAL
    assert f(FAKE, 1 << 32, 0, 0, FAKE, None) == EINVAL
    assert f(None, 3, 0, 4, FAKE, None) == EINVAL                   # calls and no table
    assert f(FAKE, 3, 0, 4, None, None) == EINVAL                   # nowhere to put them
    assert f(FAKE + 4, 3, 0, 4, FAKE, None) == EALIGN
    assert f(FAKE, 3, 0, 4, FAKE + 2, None) == EALIGN
    assert f(FAKE, 3, 7, 0, FAKE, None) == 0                        # n == 0: nothing launched
    assert f(None, 0, 7, 0, None, None) == 0


def test_pending_add_validates_before_any_hip_call():
    f = A.lib().xdrg_rpc_pending_add
    far = FAKE + (1 << 20)
    assert f(None, 3, FAKE, 4, far, None, None, None) == EINVAL
    assert f(FAKE, 3, None, 4, far, None, None, None) == EINVAL
    assert f(FAKE, 3, far, 4, None, None, None, None) == EINVAL
    assert f(FAKE, 3, far, 4, FAKE, None, None, None) == EINVAL     # merged in place of the table
    assert f(FAKE, 3, far, 4, far, None, None, None) == EINVAL      # ... of the new entries
    assert f(FAKE, 3, far, 4, FAKE + 16, None, None, None) == EINVAL  # overlapping the table
    assert f(FAKE, 3, far, 4, far - 48, None, None, None) == EINVAL   # its end inside the new entries
    assert f(FAKE + 4, 3, far, 4, 2 * far, None, None, None) == EALIGN
    assert f(FAKE, 3, far + 4, 4, 2 * far, None, None, None) == EALIGN
    assert f(FAKE, 3, far, 4, 2 * far + 4, None, None, None) == EALIGN
    assert f(FAKE, 3, far, 4, 2 * far, FAKE + 4, None, None) == EALIGN
    assert f(FAKE, 3, far, 4, 2 * far, None, FAKE + 4, None) == EALIGN
    assert f(None, 0, None, 0, None, None, None, None) == 0         # nothing to merge: nothing launched
    assert f(FAKE, 0, FAKE, 0, FAKE, FAKE, FAKE, None) == 0


def test_workspace_size():
    L = A.lib()
    ns = (1, 256, 257, 1 << 20)
    sizes = [L.xdrg_rpc_call_batch_workspace_size(n) for n in ns]
    assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
    assert sizes == sorted(sizes), sizes
    assert all(s >= 8 * n for s, n in zip(sizes, ns))  # an owner word per call


def test_python_value_errors():
    import torch
    idx = torch.zeros(1, dtype=torch.int64)
    pending = R.PendingCalls(np.zeros(0, np.uint32), np.zeros(0, np.uint32), "cpu")
    with pytest.raises(ValueError):
        R.call_batch(pending, [((1, 1, 1), 0, idx, None, None)] * 65)
    with pytest.raises(ValueError):
        R._arg_srcs([R.ArgSource((1, 1, 1), 0, idx)] * 65)
    with pytest.raises(ValueError):  # fixed-size arguments whose size cannot be taken from the bytes
        R.arg_source((1, 1, 1), 0, torch.zeros(3, dtype=torch.int64), torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        R._arg_srcs([R.ArgSource((1, 1, 1), 0, idx, None, None, 8)])
    with pytest.raises(ValueError):
        R.PendingCalls(np.array([5, 5], dtype=np.uint32), 0, "cpu", last_xid=3)
    assert R.PendingCalls([3, 1], 0, "cpu").last_xid == 0 and R.PendingCalls([3, 1], 0, "cpu", last_xid=9).last_xid == 9
    s = R.arg_source((7, 2, 1), 4, torch.zeros(2, dtype=torch.int64), torch.zeros(16, dtype=torch.uint8))
    assert (s.key, s.res, s.fixed_size, s.cap) == ((7, 2, 1), 4, 8, 2)


# ------------------------------------------- the model against the reference
@pytest.fixture(scope="module")
def batch():
    return CS.GoldenBatch()


@pytest.fixture(scope="module")
def golden(batch):
    stream, offsets, sent, counts, err = CS.model(batch.xids, batch.sources())
    assert counts == (0, 0) and err is None
    return stream, offsets, sent


def test_the_golden_batch_is_a_test(batch, golden):
    assert len(set(batch.proc.tolist())) == 61
    assert [int(np.count_nonzero(batch.kind == k)) for k in range(3)] == [353, 336, 335]
    srcs = batch.sources()
    assert len(srcs) == 61 and all(s.res == p and s.key == batch.procs[p] for p, s in enumerate(srcs))
    assert any((np.diff(s.index.astype(np.int64)) < 0).any() for s in srcs)  # shuffled
    # the xids wrap, skip pending values and a pending 0
    x = batch.xids.astype(np.int64)
    assert np.count_nonzero(np.diff(x) < 0) == 1 and np.count_nonzero(np.diff(x) > 1) >= 10
    near = ((batch.pending_xids.astype(np.int64) - batch.LAST_XID - 1) & CS.M32) < 1024
    assert np.count_nonzero(near) == 150 and 0 not in batch.xids and not np.isin(batch.xids, batch.pending_xids).any()
    stream, offsets, sent = golden
    want, want_offs = batch.expected()
    assert stream.tobytes() == want.tobytes() and np.array_equal(offsets, want_offs)
    assert np.array_equal(sent["xid"], batch.xids) and np.array_equal(sent["res"], batch.proc)


def check_headers(batch, h, stream, offsets):
    n = batch.n
    assert (h["action"] == A.RPC_DISPATCH).all() and (h["err"] == 0).all() and (h["mtype"] == 0).all()
    assert np.array_equal(h["xid"], batch.xids)
    keys = np.array([batch.procs[int(p)] for p in batch.proc], dtype=np.uint32)
    assert (h["w"][:, A.RPC_W_RPCVERS] == 2).all()
    assert np.array_equal(h["w"][:, A.RPC_W_PROG:A.RPC_W_PROC + 1], keys)
    assert (h["w"][:, A.RPC_W_CRED_FLAVOR] == 0).all() and (h["w"][:, A.RPC_W_VERF_FLAVOR] == 0).all()
    assert (h["cred_len"] == 0).all() and (h["verf_len"] == 0).all()
    assert np.array_equal(h["body_off"], offsets[:-1] + np.uint64(44)) and np.array_equal(h["end"], offsets[1:])
    for i in range(n):
        body = stream[int(h["body_off"][i]):int(h["end"][i])]
        assert body.tobytes() == batch.record(int(batch.kind[i]), i).tobytes(), i


def test_model_stream_dispatches(batch, golden):
    """(1) The server's header decode, restated in C and pinned to the
    reference by tests/test_rpc.py, reads every call of the model's stream as
    the call it is."""
    stream, offsets, _ = golden
    check_headers(batch, O.rpc_headers(stream, offsets, W.RPC_PROCS), stream, offsets)


@pytest.mark.skipif(not os.path.exists("/root/reference/xdrpp/server.h"), reason="reference tree absent")
def test_model_stream_through_the_reference(batch, golden, tmp_path):
    """(2) The reference itself -- xdr_get of rpc_msg and the real
    rpc_server_base::dispatch -- writes the same header records."""
    stream, offsets, _ = golden
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/ref_golden"], check=True)
    stream.tofile(tmp_path / "calls.bin")
    offsets.astype("<u8").tofile(tmp_path / "calls.offs")
    np.ascontiguousarray(W.RPC_PROCS, dtype="<u4").tofile(tmp_path / "procs.bin")
    pre = str(tmp_path / "out")
    subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_golden"), "rpc", str(tmp_path / "calls.bin"),
                    str(tmp_path / "calls.offs"), str(tmp_path / "procs.bin"), "-", pre], check=True)
    ref = np.fromfile(pre + ".hdrs", dtype=np.uint8)
    mine = O.rpc_headers(stream, offsets, W.RPC_PROCS)
    assert ref.tobytes() == mine.tobytes()
    check_headers(batch, ref.view(R.HDR_DTYPE), stream, offsets)


@pytest.mark.parametrize("schema", ["rec128", None])
def test_model_equals_what_call_type_marshals(schema):
    """(3) One source: the stream xdr_to_msg(hdr, args) gives through
    compile_plan(call_type(T)) and the C oracle."""
    n = 96
    key = (100003, 4, 17)
    xids = (np.arange(n, dtype=np.uint64) * 2654435761 + 11 & 0xFFFFFFFF).astype(np.uint32)
    hdr = np.zeros((n, 10), dtype="<u4")
    hdr[:, 0], hdr[:, 2] = xids, 2
    hdr[:, 3], hdr[:, 4], hdr[:, 5] = key
    index = np.arange(n, dtype=np.uint64)
    if schema is None:
        cp = compile_plan(R.call_type(None))
        want, want_offs = O.encode_msgs(cp, hdr.view(np.uint8).reshape(-1), n)
        source = CS.Src(key, 3, index)
    else:
        cp = compile_plan(R.call_type(S.ALL[schema]))
        nat, heap = W.GENERATORS[schema](n)
        rec = np.concatenate([hdr.view(np.uint8).reshape(n, 40), nat.reshape(n, cp.stride - 40)], axis=1)
        want, want_offs = O.encode_msgs(cp, rec.reshape(-1), n, heap)
        xdr, _ = O.encode(compile_plan(S.ALL[schema]), nat, n, heap)
        source = CS.Src(key, 3, index, xdr, None, xdr.size // n)
    stream, offsets, sent, counts, err = CS.model(xids, [source])
    assert stream.tobytes() == want.tobytes() and np.array_equal(offsets, want_offs)
    assert counts == (0, 0) and err is None and (sent["res"] == 3).all()


# ------------------------------------------------- the xid and merge models
@pytest.mark.parametrize("case", CS.XID_CASES, ids=[c[0] for c in CS.XID_CASES])
def test_xid_and_merge_models(case):
    """The literal get_xid loop against the search the kernel does, and
    np.argsort against the kernel's placement and against PendingCalls."""
    _, pending, last, n = case
    x = CS.next_xids(pending, last, n)
    assert np.array_equal(x, CS.next_xids_by_search(pending, last, n))
    assert np.unique(x).size == n and not np.isin(x, pending).any()
    rot = (x.astype(np.int64) - last - 1) & CS.M32
    assert (np.diff(rot) > 0).all()
    prot = (pending.astype(np.int64) - last - 1) & CS.M32
    assert int(rot[-1]) + 1 == n + np.count_nonzero(prot < rot[-1])  # the first n free values, none passed over
    rng = np.random.default_rng(n)
    old = np.sort(pending)
    old_res = rng.integers(7, size=old.size, dtype=np.int64).astype(np.uint32)
    new_res = (np.arange(n) % 5).astype(np.uint32)
    table, old_pos, new_pos = CS.merge(old, old_res, x, new_res)
    assert (np.diff(table["xid"].astype(np.int64)) > 0).all()
    so, sn = CS.merge_by_search(old, x)
    assert np.array_equal(so, old_pos) and np.array_equal(sn, new_pos)
    p = R.PendingCalls(np.concatenate([old, x]), np.concatenate([old_res, new_res]), "cpu")
    assert np.array_equal(p.calls, table)
    assert np.array_equal(p.inv.numpy().astype(np.uint64), np.concatenate([old_pos, new_pos]))


def test_xid_search_on_random_tables():
    rng = np.random.default_rng(5)
    for _ in range(200):
        last = int(rng.choice([0, 0xFFFFFFFF, 0xFFFFFFF0, int(rng.integers(1 << 32))]))
        near = (last + 1 + rng.integers(0, 120, size=int(rng.integers(0, 80)))) & CS.M32
        far = rng.integers(1 << 32, size=int(rng.integers(0, 20)))
        pending = np.unique(np.concatenate([near, far]).astype(np.uint32))
        n = int(rng.integers(1, 100))
        x = CS.next_xids(pending, last, n)
        assert np.array_equal(x, CS.next_xids_by_search(pending, last, n))
        so, sn = CS.merge_by_search(pending, x)
        _, old_pos, new_pos = CS.merge(pending, np.zeros(pending.size), x, np.zeros(n))
        assert np.array_equal(so, old_pos) and np.array_equal(sn, new_pos)
