"""CPU: the host side of the asynchronous client's reply calls
(include/xdrgpu.h "Asynchronous client replies": xdrg_rpc_match_replies,
xdrg_rpc_verify_results, xdrg_rpc_gather_results): the xdrg_rpc_call layout
and the new status values read from the header, the argument validation that
runs before any HIP call, call_type against the restatement's server-side
header decode, PendingCalls, and the mixed reply batch of
test_gpu_rpc_results.py as a test (the model alone: no GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import marshal as M
from xdrpp_amd import rpc as R
from xdrpp_amd import schemas as S
from xdrpp_amd import workloads as W
from xdrpp_amd.xdr_types import compile_plan
import oracle_bridge as O
import reply_batches as RB

EINVAL, EALIGN = -1, -2
FAKE = 0x10000  # a nonzero, 64 KiB-aligned address no call may dereference

LAYOUT_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "xdrgpu.h"
int main(void) {
  printf("sizeof %zu\n", sizeof(xdrg_rpc_call));
  printf("xid %zu\n", offsetof(xdrg_rpc_call, xid));
  printf("res %zu\n", offsetof(xdrg_rpc_call, res));
  printf("UNKNOWN_XID %d\n", (int)XDRG_RPCR_UNKNOWN_XID);
  printf("GARBAGE_RES %d\n", (int)XDRG_RPCR_GARBAGE_RES);
  printf("BAD_XID %d\n", (int)XDRG_RPCR_BAD_XID);
  printf("NO_CALL %d\n", XDRG_RPC_NO_CALL == 0xffffffffffffffffull && sizeof(XDRG_RPC_NO_CALL) == 8);
  printf("ABI %d\n", XDRG_ABI_VERSION);
  return 0;
}
"""


def test_call_layout_and_status_values(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(LAYOUT_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["sizeof"] == C.sizeof(A.XdrgRpcCall) == R.CALL_DTYPE.itemsize == A.RPC_CALL_BYTES == 8
    assert got["xid"] == A.XdrgRpcCall.xid.offset == 0 and got["res"] == A.XdrgRpcCall.res.offset == 4
    assert got["UNKNOWN_XID"] == A.RPCR_UNKNOWN_XID == 7
    assert got["GARBAGE_RES"] == A.RPCR_GARBAGE_RES == 8
    assert got["BAD_XID"] == A.RPCR_BAD_XID == 6
    assert got["NO_CALL"] == 1 and A.RPC_NO_CALL == (1 << 64) - 1
    assert got["ABI"] == A.ABI_VERSION == A.lib().xdrg_abi_version() == 10


# ------------------------------------------------------- host validation
def match(n=4, ncalls=4, stream=FAKE, offsets=FAKE, calls=FAKE, hdrs=FAKE, call=FAKE, reply_of=FAKE):
    return A.lib().xdrg_rpc_match_replies(stream, 1024, offsets, n, calls, ncalls, hdrs, call, reply_of, None)


def test_match_replies_validates_before_any_hip_call():
    for name in ("stream", "offsets", "hdrs", "call"):
        assert match(**{name: None}) == EINVAL, name
        assert match(ncalls=0, calls=None, reply_of=None, **{name: None}) == EINVAL, name
    assert match(calls=None) == EINVAL and match(reply_of=None) == EINVAL
    assert match(n=0, calls=None) == EINVAL and match(n=0, reply_of=None) == EINVAL
    assert match(stream=FAKE + 2) == EALIGN
    assert match(offsets=FAKE + 4) == EALIGN
    assert match(calls=FAKE + 4) == EALIGN
    assert match(hdrs=FAKE + 8) == EALIGN
    assert match(call=FAKE + 4) == EALIGN
    assert match(reply_of=FAKE + 4) == EALIGN
    # nothing to do: OK, nothing launched
    assert match(n=0, ncalls=0) == A.OK
    assert match(n=0, ncalls=0, stream=None, offsets=None, calls=None, hdrs=None, call=None, reply_of=None) == A.OK


def plan_array(handles):
    return (C.c_void_p * max(len(handles), 1))(*handles)


def verify_results(n=4, ncalls=4, handles=(None,), nplans=None, stream=FAKE, hdrs=FAKE, call=FAKE, calls=FAKE,
                   verdicts=None, plans=True):
    arr = plan_array(list(handles)) if plans else None
    return A.lib().xdrg_rpc_verify_results(stream, 1024, hdrs, call, n, calls, ncalls, arr,
                                           len(handles) if nplans is None else nplans, 0,
                                           A.DEFAULT_STACK_LIMIT, verdicts, None)


def test_verify_results_validates_before_any_hip_call():
    assert verify_results(handles=[None] * 65) == EINVAL          # more than 64 result types
    assert verify_results(handles=[None] * 65, n=0) == EINVAL
    assert verify_results(nplans=1, plans=False) == EINVAL        # no table
    for name in ("stream", "hdrs", "call", "calls"):
        assert verify_results(**{name: None}) == EINVAL, name
    assert verify_results(stream=FAKE + 1) == EALIGN
    assert verify_results(hdrs=FAKE + 8) == EALIGN
    assert verify_results(call=FAKE + 4) == EALIGN
    assert verify_results(calls=FAKE + 4) == EALIGN
    assert verify_results(verdicts=FAKE + 2) == EALIGN
    # an empty batch: OK, nothing launched, whatever the plans
    assert verify_results(n=0, ncalls=0, handles=[None] * 64) == A.OK
    assert verify_results(n=0, ncalls=0, handles=[], stream=None, hdrs=None, call=None, calls=None) == A.OK
    plan = M.Plan(S.recvar)
    assert verify_results(n=0, handles=[plan.handle, None]) == A.OK


def gather_results(n=4, ncalls=4, stream=FAKE, hdrs=FAKE, call=FAKE, calls=FAKE, out=FAKE, cap=64, offsets=FAKE,
                   index=FAKE, count=FAKE, ws=FAKE, ws_bytes=1 << 20, status=FAKE):
    return A.lib().xdrg_rpc_gather_results(stream, 1024, hdrs, call, n, calls, ncalls, 0, out, cap, offsets, index,
                                           count, ws, ws_bytes, status, None)


def test_gather_results_validates_before_any_hip_call():
    for name in ("offsets", "count", "status"):
        assert gather_results(**{name: None}) == EINVAL, name
        assert gather_results(n=0, **{name: None}) == EINVAL, name
    for name in ("stream", "hdrs", "call", "calls", "index", "out"):
        assert gather_results(**{name: None}) == EINVAL, name
    assert gather_results(hdrs=FAKE + 8) == EALIGN
    for name in ("call", "calls", "offsets", "index", "count", "ws"):
        assert gather_results(**{name: FAKE + 4}) == EALIGN, name
    assert gather_results(ws_bytes=8) == -6  # XDRG_ESPACE
    L = A.lib()
    for n in (0, 1, 256, 257, 1 << 20):
        assert L.xdrg_rpc_gather_results_workspace_size(n) == L.xdrg_rpc_gather_workspace_size(n)


# ------------------------------------------------------------ call_type
def test_call_type_is_what_the_server_dispatches():
    """compile_plan(call_type(rec128)) encoded by the restatement and read
    back by its server-side header decode: DISPATCH with the staged xid,
    prog, vers and proc, the arguments at mark + 44."""
    cp = compile_plan(R.call_type(S.ALL["rec128"]))
    n = 64
    args, _ = W.rec128(n)
    assert cp.stride == 40 + 128
    key = tuple(int(v) for v in W.RPC_PROCS[W.RPC_PROCS[:, 3] == 0][5][:3])
    hdr = np.zeros((n, 10), dtype="<u4")
    hdr[:, 0] = (np.arange(n, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    hdr[:, 2] = 2
    hdr[:, 3], hdr[:, 4], hdr[:, 5] = key
    nat = np.concatenate([hdr.view(np.uint8).reshape(n, 40), args.reshape(n, 128)], axis=1).reshape(-1)
    stream, offs = O.encode_msgs(cp, nat, n)
    h = O.rpc_headers(stream, offs, W.RPC_PROCS)
    assert (h["action"] == A.RPC_DISPATCH).all() and (h["err"] == 0).all()
    assert np.array_equal(h["xid"], hdr[:, 0])
    assert (h["w"][:, A.RPC_W_RPCVERS] == 2).all()
    assert np.array_equal(h["w"][:, 1:4], np.tile(np.array(key, dtype=np.uint32), (n, 1)))
    assert np.array_equal(h["body_off"], offs[:-1] + 44) and np.array_equal(h["end"], offs[1:])
    ref, _ = O.encode(compile_plan(S.ALL["rec128"]), args, n)  # the arguments follow, as encoded alone
    got = np.stack([stream[int(h["body_off"][i]):int(h["end"][i])] for i in range(n)])
    assert np.array_equal(got.reshape(-1), ref)
    # a procedure without arguments: the header alone
    cp0 = compile_plan(R.call_type(None))
    s0, o0 = O.encode_msgs(cp0, hdr.view(np.uint8).reshape(-1), n)
    h0 = O.rpc_headers(s0, o0, W.RPC_PROCS)
    assert cp0.stride == 40 and (h0["action"] == A.RPC_DISPATCH).all()
    assert np.array_equal(h0["body_off"], o0[1:]) and np.array_equal(h0["body_off"], o0[:-1] + 44)


# --------------------------------------------------------- PendingCalls
def test_pending_calls_sorts_unsigned_and_keeps_positions():
    xids = np.array([0x80000000, 5, 0xFFFFFFFF, 0, 0x7FFFFFFF, 77], dtype=np.uint32)
    res = np.array([3, 1, 4, 1, 5, 9], dtype=np.uint32)
    p = R.PendingCalls(xids, res, device="cpu")
    t = p.table.numpy().view(R.CALL_DTYPE)
    assert t["xid"].tolist() == [0, 5, 77, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    assert t["res"].tolist() == [1, 1, 9, 5, 3, 4]
    assert p.ncalls == 6 and p.table.data_ptr() % 8 == 0
    assert np.array_equal(xids[p.perm.numpy()], t["xid"])
    assert np.array_equal(p.inv.numpy()[p.perm.numpy()], np.arange(6))
    import torch
    tab = torch.tensor([0, -1, 5, 4, -1], dtype=torch.int64)
    assert p.to_caller(tab).tolist() == [3, -1, 2, 0, -1]
    assert p.to_table(p.to_caller(tab)).tolist() == tab.tolist()
    # xids given as negative int32 are the same words
    q = R.PendingCalls(xids.view(np.int32), 2, device="cpu")
    assert np.array_equal(q.table.numpy().view(R.CALL_DTYPE)["xid"], t["xid"])
    assert (q.table.numpy().view(R.CALL_DTYPE)["res"] == 2).all()
    e = R.PendingCalls(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), device="cpu")
    assert e.ncalls == 0 and e.to_caller(tab[:2]).tolist() == [0, -1]


def test_pending_calls_refuses_a_duplicate_xid():
    with pytest.raises(ValueError):
        R.PendingCalls([7, 9, 7], [0, 0, 0], device="cpu")
    with pytest.raises(ValueError):  # the same word, signed and unsigned
        R.PendingCalls(np.array([-1, 0xFFFFFFFF], dtype=np.int64), 0, device="cpu")


def test_python_verify_results_splits_result_types_into_runs():
    plans = {k: None for k in list(range(70)) + [100, 101, 200]}
    runs = R._res_runs(plans)
    assert [(r[0], len(r)) for r in runs] == [(0, 64), (64, 6), (100, 2), (200, 1)]


def test_call_stat_message():
    h = np.zeros(1, dtype=R.HDR_DTYPE)[0]
    h["action"] = A.RPCR_GARBAGE_RES
    assert R.call_stat_message(h) == "unable to unmarshal reply value sent by server"
    h["action"] = A.RPCR_MALFORMED
    assert R.call_stat_message(h) == "unable to unmarshal reply value sent by server"
    h["action"], h["w"][A.RPC_W_STAT] = A.RPCR_ACCEPT_STAT, 4
    assert R.call_stat_message(h) == "procedure can't decode params"
    h["action"], h["w"][A.RPC_W_WHY] = A.RPCR_AUTH_STAT, 5
    assert R.call_stat_message(h) == "rejected for security reasons"
    h["action"] = A.RPCR_RPCVERS_MISMATCH
    assert R.call_stat_message(h) == "server reported rpcvers field with wrong value"
    h["action"] = A.RPCR_OK
    assert R.call_stat_message(h) == "RPC executed successfully"
    h["action"] = A.RPCR_UNKNOWN_XID
    with pytest.raises(ValueError):
        R.call_stat_message(h)


# ----------------------------------------------- the mixed batch is a test
@pytest.fixture(scope="module")
def batch():
    return RB.MixedBatch()


def test_the_mixed_batch_is_a_test(batch):
    """On the model alone: every status these calls can leave occurs (BAD_XID
    needs d_xids, which match_replies does not pass), several different
    errors, and the damage splits the matched OK replies."""
    acts = set(batch.model["action"].tolist())
    assert acts == {A.RPCR_OK, A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH, A.RPCR_NOT_REPLY,
                    A.RPCR_MALFORMED, A.RPCR_UNKNOWN_XID, A.RPCR_GARBAGE_RES}, acts
    assert len({int(v) & 0xFF for v in batch.verdicts if v}) >= 3
    served = np.array([c >= 0 and int(batch.res[c]) in batch.cps for c in batch.call])
    ok = served & (batch.matched["action"] == A.RPCR_OK)
    bad = np.count_nonzero(batch.verdicts[ok])
    print("matched OK replies", np.count_nonzero(ok), "of them failing", bad)
    assert 0.10 * np.count_nonzero(ok) <= bad <= 0.60 * np.count_nonzero(ok)
    for r in RB.RES:  # every result type has replies left to gather, and failures
        sel = batch.selected(r)
        failed = np.count_nonzero(batch.verdicts[(batch.call >= 0) & (batch.res[np.clip(batch.call, 0, None)] == r)])
        assert len(sel) >= 48 and failed >= 4, (r, len(sel), failed)
    # error replies: some clean (untouched), some with trailing bytes (GARBAGE_RES, TRAILING)
    err = np.isin(batch.matched["action"], (A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH)) & served
    assert np.count_nonzero(batch.verdicts[err]) >= 8 and np.count_nonzero(batch.verdicts[err] == 0) >= 8
    # calls never answered, replies to no call, a result type nobody serves
    assert np.count_nonzero(batch.reply_of < 0) >= 16
    assert np.count_nonzero(batch.matched["action"] == A.RPCR_UNKNOWN_XID) >= 32
    unserved = (batch.call >= 0) & ~served
    assert np.count_nonzero(unserved) >= 32 and not batch.verdicts[unserved].any()
    assert batch.model[unserved].tobytes() == batch.matched[unserved].tobytes()
