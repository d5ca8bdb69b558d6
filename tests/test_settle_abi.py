"""CPU: the host side of settling a reply batch (include/xdrgpu.h "Settling a
reply batch"): the xdrg_rpc_call_stat layout and the XDRG_RPCS_* values read
from the header, the argument validation of xdrg_rpc_call_stats and
xdrg_rpc_pending_retire that runs before any HIP call, the workspace size, the
two formulations of settle_model against each other and against
PendingCalls, and the model's stats on the reference's own reply bytes.  No
GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
from xdrpp_amd import schemas as S
from xdrpp_amd.xdr_types import compile_plan
import call_stream_model as CS
import reply_model as RM
import settle_model as SM

EINVAL, EALIGN, EUNSUPPORTED, ESPACE = -1, -2, -3, -6
FAKE = 0x10000  # a nonzero, 64 KiB-aligned address no call may dereference
FAR = FAKE + (1 << 20)
PENDING, NETWORK_ERROR = A.RPCS_PENDING, A.RPCS_NETWORK_ERROR

HEADER_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "xdrgpu.h"
int main(void) {
  printf("sizeof %zu\n", sizeof(xdrg_rpc_call_stat));
  printf("type %zu\n", offsetof(xdrg_rpc_call_stat, type));
  printf("stat %zu\n", offsetof(xdrg_rpc_call_stat, stat));
  printf("ACCEPT_STAT %u\n", XDRG_RPCS_ACCEPT_STAT);
  printf("AUTH_STAT %u\n", XDRG_RPCS_AUTH_STAT);
  printf("RPCVERS_MISMATCH %u\n", XDRG_RPCS_RPCVERS_MISMATCH);
  printf("GARBAGE_RES %u\n", XDRG_RPCS_GARBAGE_RES);
  printf("NETWORK_ERROR %u\n", XDRG_RPCS_NETWORK_ERROR);
  printf("BAD_ALLOC %u\n", XDRG_RPCS_BAD_ALLOC);
  printf("PENDING %u\n", XDRG_RPCS_PENDING);
  printf("ABI %d\n", XDRG_ABI_VERSION);
  return 0;
}
"""


def test_header_facts(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(HEADER_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["sizeof"] == A.RPC_CALL_STAT_BYTES == A.CALL_STAT_DTYPE.itemsize == 8
    assert (got["type"], got["stat"]) == (0, 4) == tuple(A.CALL_STAT_DTYPE.fields[f][1] for f in ("type", "stat"))
    # rpc_call_stat::stat_type in the reference's order (exception.h:29-36)
    want = {"ACCEPT_STAT": 0, "AUTH_STAT": 1, "RPCVERS_MISMATCH": 2, "GARBAGE_RES": 3, "NETWORK_ERROR": 4,
            "BAD_ALLOC": 5, "PENDING": 0xFFFFFFFF}
    for k, v in want.items():
        assert got[k] == getattr(A, "RPCS_" + k) == v, k
    assert got["ABI"] == A.ABI_VERSION == A.lib().xdrg_abi_version() == 10
    assert R.CALL_STAT_DTYPE is A.CALL_STAT_DTYPE


# ------------------------------------------------------- host validation
def test_call_stats_validates_before_any_hip_call():
    f = A.lib().xdrg_rpc_call_stats
    for bad in (0, 3, 5, 0xFFFFFFFE):  # unanswered is PENDING or NETWORK_ERROR
        assert f(FAKE, 4, FAR, 3, bad, 2 * FAR, None) == EINVAL
        assert f(None, 0, None, 0, bad, None, None) == EINVAL
    for un in (PENDING, NETWORK_ERROR):
        assert f(FAKE, 4, None, 3, un, 2 * FAR, None) == EINVAL   # no reply_of
        assert f(FAKE, 4, FAR, 3, un, None, None) == EINVAL       # nowhere to put the stats
        assert f(None, 4, FAR, 3, un, 2 * FAR, None) == EINVAL    # messages and no headers
        assert f(FAKE + 8, 4, FAR, 3, un, 2 * FAR, None) == EALIGN  # headers: 16
        assert f(FAKE, 4, FAR + 4, 3, un, 2 * FAR, None) == EALIGN
        assert f(FAKE, 4, FAR, 3, un, 2 * FAR + 4, None) == EALIGN
        assert f(FAKE, 4, FAR, (0x7FFFFFFF << 8) + 1, un, 2 * FAR, None) == EUNSUPPORTED  # one workgroup too many
        assert f(FAKE, 4, FAR, 0, un, 2 * FAR, None) == 0         # ncalls == 0: nothing launched
        assert f(None, 0, None, 0, un, None, None) == 0
        assert f(None, 4, None, 0, un, None, None) == 0


def retire(calls=FAKE, ncalls=3, reply_of=FAR, kept=2 * FAR, kept_pos=None, count=3 * FAR, ws=4 * FAR,
           ws_bytes=1 << 40):
    return A.lib().xdrg_rpc_pending_retire(calls, ncalls, reply_of, kept, kept_pos, count, ws, ws_bytes, None)


def test_pending_retire_validates_before_any_hip_call():
    assert retire(calls=None) == EINVAL
    assert retire(reply_of=None) == EINVAL
    assert retire(kept=None) == EINVAL
    assert retire(count=None) == EINVAL
    assert retire(ncalls=0, count=None) == EINVAL             # the count is written even for an empty table
    # d_kept against d_calls: equal, overlapping from either side, and just clear of it
    assert retire(kept=FAKE) == EINVAL
    assert retire(kept=FAKE + 16) == EINVAL
    assert retire(kept=FAKE - 16) == EINVAL
    assert retire(ncalls=1000, kept=FAKE + 8 * 999) == EINVAL
    assert retire(ncalls=1000, kept=FAKE - 8 * 999) == EINVAL
    assert retire(kept=FAKE + 24, ws_bytes=0) == ESPACE        # adjacent: legal
    assert retire(kept=FAKE - 24, ws_bytes=0) == ESPACE
    # alignment: every array 8
    assert retire(calls=FAKE + 4) == EALIGN
    assert retire(reply_of=FAR + 4) == EALIGN
    assert retire(kept=2 * FAR + 4) == EALIGN
    assert retire(kept_pos=FAKE + 4) == EALIGN
    assert retire(count=3 * FAR + 4) == EALIGN
    assert retire(ws=4 * FAR + 4) == EALIGN
    assert retire(kept_pos=5 * FAR, ws_bytes=0) == ESPACE      # aligned enough
    # workspace
    need = A.lib().xdrg_rpc_pending_retire_workspace_size
    assert retire(ws_bytes=need(3) - 1) == ESPACE and retire(ws=None) == ESPACE
    assert retire(ncalls=257, kept=1 << 40, ws_bytes=need(257) - 1) == ESPACE
    # the grid: 0x7fffffff tiles are the most
    big = (0x7FFFFFFF << 8) + 1
    assert retire(ncalls=big, kept=1 << 50, ws_bytes=need(big)) == EUNSUPPORTED
    assert retire(ncalls=big - 1, kept=1 << 50, ws_bytes=need(big - 1) - 1) == ESPACE
    assert retire(ncalls=1 << 62, kept=1 << 50) == EUNSUPPORTED


def test_workspace_size():
    need = A.lib().xdrg_rpc_pending_retire_workspace_size
    ns = (0, 1, 256, 257, 1 << 16, SM.TILE * SM.SCAN_LANES + 1, 1 << 31)
    sizes = [need(n) for n in ns]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes), sizes
    assert all(s >= 8 * ((n + SM.TILE - 1) // SM.TILE) for s, n in zip(sizes, ns))  # a count per tile
    assert sizes[1] > 0 and sizes[-2] > sizes[-3]


def test_python_surface():
    import torch
    assert R.call_stat_text(A.RPCS_ACCEPT_STAT, 0) == "RPC executed successfully" == R.rpc_errmsg_accept(0)
    assert R.call_stat_text(A.RPCS_ACCEPT_STAT, 4) == R.rpc_errmsg_accept(4) == "procedure can't decode params"
    assert R.call_stat_text(A.RPCS_AUTH_STAT, 5) == R.rpc_errmsg_auth(5)
    assert R.call_stat_text(A.RPCS_RPCVERS_MISMATCH, 0) == "server reported rpcvers field with wrong value"
    assert R.call_stat_text(A.RPCS_GARBAGE_RES, 0) == "unable to unmarshal reply value sent by server"
    assert R.call_stat_text(A.RPCS_NETWORK_ERROR) == "network error when communicating with server"
    assert R.call_stat_text(A.RPCS_BAD_ALLOC) == "insufficient memory to unmarshal result"
    with pytest.raises(ValueError):
        R.call_stat_text(A.RPCS_PENDING, 0)
    with pytest.raises(ValueError):
        R.call_stat_text(17, 0)
    # the same table as call_stat_message
    h = np.zeros(5, dtype=R.HDR_DTYPE)
    h["action"] = [A.RPCR_OK, A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH, A.RPCR_MALFORMED]
    h["w"][:, A.RPC_W_STAT], h["w"][:, A.RPC_W_WHY] = 3, 6
    for r in h:
        assert R.call_stat_text(*SM.call_stat(r)) == R.call_stat_message(r)
    s = torch.from_numpy(np.array([(1, 5), (0xFFFFFFFF, 0)], dtype=A.CALL_STAT_DTYPE).view(np.int64).copy())
    assert R.call_stats_numpy(s).tolist() == [(1, 5), (0xFFFFFFFF, 0)]
    # the empty table retires to the empty table without a launch
    p = R.PendingCalls(np.zeros(0, np.uint32), np.zeros(0, np.uint32), "cpu", last_xid=77)
    q, old = p.retire(torch.zeros(0, dtype=torch.int64))
    assert q.ncalls == 0 and old.numel() == 0 and q.last_xid == 77


# ------------------------------------------------------ model consistency
def check_one(xids, res, reply_of):
    """The dict walk, the array form and PendingCalls(survivors) on one table;
    reply_of in the caller's order."""
    table, perm = SM.sorted_table(xids, res)
    kept, kept_pos, count, tile_base = SM.retire_arrays(table, SM.to_table_order(reply_of, perm))
    lit_table, old_of_new, inv = SM.retire(xids, res, reply_of)
    assert count == len(lit_table) == len(old_of_new) and np.array_equal(kept, lit_table)
    assert len(tile_base) == (len(xids) + SM.TILE - 1) // SM.TILE
    # d_kept_pos[pending.inv[old_of_new]]: the new table position of every surviving call
    p_inv = np.empty(len(xids), dtype=np.int64)
    p_inv[perm] = np.arange(len(xids))
    assert np.array_equal(kept_pos[p_inv[old_of_new]], inv.astype(np.uint64))
    retired = np.setdiff1d(np.arange(len(xids)), old_of_new)
    assert (kept_pos[p_inv[retired]] == SM.NO_CALL).all()
    q = R.PendingCalls(np.asarray(xids)[old_of_new], np.asarray(res)[old_of_new], "cpu")
    assert np.array_equal(q.calls, lit_table) and np.array_equal(q.inv.numpy(), inv)
    return count


@pytest.mark.parametrize("nc", SM.SIZES)
def test_models_agree_on_the_gpu_cases(nc):
    xids, res = SM.case_table(nc)
    table, perm = SM.sorted_table(xids, res)
    counts = {}
    for name in SM.MASKS:
        rt = SM.answered_values(SM.answered_mask(name, nc))
        reply_of = np.empty(nc, dtype=np.int64)
        reply_of[perm] = rt.view(np.int64)
        counts[name] = check_one(xids, res, reply_of)
    assert counts["none"] == nc and counts["all"] == 0
    assert counts["first_of_wave"] + counts["kept_first_of_wave"] == nc


def test_models_agree_on_random_tables():
    rng = np.random.default_rng(6)
    for _ in range(200):
        nc = int(rng.integers(0, 700))
        xids = np.unique(rng.integers(1 << 32, size=nc, dtype=np.int64).astype(np.uint32))
        xids = rng.permutation(xids)
        res = rng.integers(9, size=xids.size)
        p = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0]))
        reply_of = np.where(rng.random(xids.size) < p, rng.integers(0, 1 << 40, size=xids.size), -1)
        check_one(xids, res, reply_of)


def test_answered_values_keep_the_mask():
    for name in SM.MASKS:
        mask = SM.answered_mask(name, 1025)
        v = SM.answered_values(mask)
        assert np.array_equal(v != SM.NO_CALL, mask)
    v = SM.answered_values(np.ones(1025, dtype=bool))
    assert np.count_nonzero(v >= 1000) >= 100 and np.count_nonzero(v < 1000) >= 100  # both sorts of answered


# ------------------------------------------- stats on the reference's bytes
def g(name, dtype=np.uint8):
    return np.fromfile(os.path.join(GOLD, name), dtype=dtype)


def golden_replies():
    """rpc_1024.msgs matched as test_gpu_rpc_results.test_all_reply_kinds
    does: the pending table is every second reply's xid."""
    m, mo = g("rpc_1024.msgs"), g("rpc_1024.msgoffs", "<u8")
    n = mo.size - 1
    words = np.array([[RM.be_word(m, int(mo[i]) + 4), RM.be_word(m, int(mo[i]) + 8)] if mo[i + 1] - mo[i] >= 12
                      else [0, 0xFFFFFFFF] for i in range(n)], dtype=np.uint64)
    replies = np.nonzero(words[:, 1] == 1)[0]
    assert replies.size == 481
    return m, mo, words[replies[::2], 0].astype(np.uint32)


@pytest.mark.parametrize("result", ["void", "rec128", "mixed"])
def test_stats_on_the_reference_bytes(result):
    """void and rec128 as test_all_reply_kinds has them; "mixed": every
    second call expects a rec128, so that one batch shows every kind."""
    m, mo, xids = golden_replies()
    chk = g("rpc_1024.chk").view(R.HDR_DTYPE)
    res = {"void": np.zeros(xids.size, np.uint32), "rec128": np.ones(xids.size, np.uint32),
           "mixed": (np.arange(xids.size) % 2).astype(np.uint32)}[result]
    cps = {0: None, 1: compile_plan(S.rec128)}
    matched, _, _ = RM.match(m, mo, xids)
    hdrs, call, reply_of, stats, (table, old_of_new, inv) = SM.settle(m, mo, xids, res, cps)
    # the headers the stats are read from are the reference's own, with the join's and the result decode's rewrites
    expect = chk.copy()
    expect["action"][chk["action"] == A.RPCR_BAD_XID] = A.RPCR_OK
    expect["action"][matched["action"] == A.RPCR_UNKNOWN_XID] = A.RPCR_UNKNOWN_XID
    assert expect.tobytes() == matched.tobytes()
    assert (reply_of >= 0).all() and len(table) == 0 and len(old_of_new) == 0  # every call answered: calls_ is empty
    by = chk[reply_of]  # the reference-decoded header of the reply each call got
    ty, st = stats["type"], stats["stat"]
    ok = by["action"] == A.RPCR_OK
    bad_xid = by["action"] == A.RPCR_BAD_XID  # the synchronous client's xid test: successes here
    acc = by["action"] == A.RPCR_ACCEPT_STAT
    auth = by["action"] == A.RPCR_AUTH_STAT
    vers = by["action"] == A.RPCR_RPCVERS_MISMATCH
    other = ~(ok | bad_xid | acc | auth | vers)
    success = (ty == A.RPCS_ACCEPT_STAT) & (st == 0)
    garbage = (ty == A.RPCS_GARBAGE_RES) & (st == 0)
    void = res == 0
    assert success[(ok | bad_xid) & void].all() and not success[~void].any()
    assert garbage[(ok | bad_xid) & ~void].all()  # a bodiless success does not hold a rec128
    assert np.count_nonzero(ok | bad_xid) >= 16
    still = hdrs["action"][reply_of] != A.RPCR_GARBAGE_RES  # not turned over by g.done()
    assert (ty[acc & still] == A.RPCS_ACCEPT_STAT).all() and np.array_equal(st[acc & still], by["w"][acc & still, 1])
    assert (st[acc & still] != 0).all() and len(set(st[acc & still].tolist())) >= 2
    assert (ty[auth & still] == A.RPCS_AUTH_STAT).all() and np.array_equal(st[auth & still], by["w"][auth & still, 2])
    assert (ty[vers & still] == A.RPCS_RPCVERS_MISMATCH).all() and (st[vers & still] == 0).all()
    assert garbage[other].all() and garbage[~still].all()
    for kind in (acc & still, auth & still, vers & still):
        assert kind.any()
    assert success.any() or result == "rec128"
    assert garbage.any() or result == "void"
    if result == "mixed":  # every kind at least once in one batch
        kinds = [success, (ty == A.RPCS_ACCEPT_STAT) & (st != 0), (ty == A.RPCS_AUTH_STAT) & (st != 0),
                 ty == A.RPCS_RPCVERS_MISMATCH, garbage]
        assert all(k.any() for k in kinds) and np.logical_or.reduce(kinds).all()
    for s in stats[:32]:
        R.call_stat_text(int(s["type"]), int(s["stat"]))
    # aborted: nobody was outstanding, so nothing changes
    assert np.array_equal(SM.settle(m, mo, xids, res, cps, aborted=True)[3], stats)


def test_stats_of_the_unanswered_and_the_out_of_range():
    h = np.zeros(3, dtype=R.HDR_DTYPE)
    h["action"] = [A.RPCR_OK, A.RPCR_AUTH_STAT, A.RPCR_UNKNOWN_XID]
    h["w"][:, A.RPC_W_WHY] = 9
    reply_of = np.array([-1, 0, 1, 2, 3, 1 << 40, -2], dtype=np.int64)
    want = [(A.RPCS_PENDING, 0), (0, 0), (A.RPCS_AUTH_STAT, 9)] + [(A.RPCS_GARBAGE_RES, 0)] * 4
    assert SM.call_stats(h, reply_of).tolist() == want
    want[0] = (A.RPCS_NETWORK_ERROR, 0)
    assert SM.call_stats(h, reply_of, aborted=True).tolist() == want


def test_next_xids_after_the_erases():
    """get_xid skips only what is in calls_ now: after a wrap the retired
    xids are handed out again."""
    xids = CS._run(0xFFFFFFF0, 40)
    reply_of = np.where(np.arange(40) % 2 == 0, np.arange(40), -1)
    got = SM.next_xids(xids, reply_of, 0xFFFFFFEF, 30)
    assert np.array_equal(got[:6], xids[[0, 2, 4, 6, 8, 10]])
    assert 0 in got.tolist() or 0 in xids[1::2].tolist()
    assert not np.isin(got, xids[1::2]).any()
    assert not np.array_equal(got, CS.next_xids(xids, 0xFFFFFFEF, 30))  # the unretired table gives other xids
