"""CPU: the host side of the many-socket client calls (include/xdrgpu.h "The
asynchronous client over many connections"): the prototypes and the ABI number
from a compiled C snippet, every validation rule with addresses no call may
dereference, the workspace size, SockCalls against PendingCalls socket by
socket, and socks_model against the single-socket models on the tables the GPU
tests use.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R
import call_stream_model as CS
import settle_model as SM
import socks_model as KM

EINVAL, EALIGN, EUNSUPPORTED, ESPACE = -1, -2, -3, -6
FAKE = 0x10000  # a nonzero, 64 KiB-aligned address no call may dereference
FAR = 1 << 20
BIG = (0x7FFFFFFF << 8) + 1  # one workgroup too many

PROTO_PROBE = r"""
#include <stdio.h>
#include "xdrgpu.h"
/* assigning to these pointer types fails to compile if a prototype differs */
int (*p1)(const xdrg_rpc_call *, const uint32_t *, uint64_t, const uint32_t *, uint64_t, const uint32_t *, uint64_t,
          uint32_t *, uint32_t *, void *) = xdrg_rpc_socks_next_xids;
int (*p2)(const xdrg_rpc_call *, const uint32_t *, uint64_t, const xdrg_rpc_call *, const uint32_t *, uint64_t,
          xdrg_rpc_call *, uint32_t *, uint64_t *, uint64_t *, void *) = xdrg_rpc_socks_pending_add;
int (*p3)(const void *, uint64_t, const uint64_t *, uint64_t, const uint32_t *, const uint32_t *, uint64_t,
          const xdrg_rpc_call *, const uint32_t *, uint64_t, xdrg_rpc_hdr *, uint64_t *, uint64_t *, void *) =
    xdrg_rpc_socks_match_replies;
int (*p4)(const xdrg_rpc_hdr *, uint64_t, const uint64_t *, const uint32_t *, uint64_t, const uint32_t *, uint64_t,
          xdrg_rpc_call_stat *, void *) = xdrg_rpc_socks_call_stats;
int (*p5)(const xdrg_rpc_call *, const uint32_t *, uint64_t, const uint64_t *, const uint32_t *, uint64_t,
          xdrg_rpc_call *, uint32_t *, uint64_t *, uint64_t *, void *, size_t, void *) = xdrg_rpc_socks_pending_retire;
size_t (*p6)(uint64_t) = xdrg_rpc_socks_pending_retire_workspace_size;
int main(void) {
  printf("ABI %d\n", XDRG_ABI_VERSION);
  printf("call %zu\n", sizeof(xdrg_rpc_call));
  return 0;
}
"""


def test_prototypes_and_abi(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROTO_PROBE)
    obj = tmp_path / "probe.o"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(obj),
                    str(src)], check=True)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-o", str(exe), str(obj), A.lib()._name, "-Wl,-rpath," + os.path.dirname(A.lib()._name)],
                   check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(got["ABI"]) == A.ABI_VERSION == A.lib().xdrg_abi_version() == 10
    assert int(got["call"]) == A.RPC_CALL_BYTES == 8
    for name in ("xdrg_rpc_socks_next_xids", "xdrg_rpc_socks_pending_add", "xdrg_rpc_socks_match_replies",
                 "xdrg_rpc_socks_call_stats", "xdrg_rpc_socks_pending_retire",
                 "xdrg_rpc_socks_pending_retire_workspace_size"):
        assert name in A.EXPORTED and getattr(A.lib(), name)


# ------------------------------------------------------- host validation
def nx(calls=FAKE, sock=FAKE + FAR, ncalls=3, last=FAKE + 2 * FAR, nsocks=4, call_sock=FAKE + 3 * FAR, n=5,
       xids=FAKE + 4 * FAR, last_out=FAKE + 5 * FAR):
    return A.lib().xdrg_rpc_socks_next_xids(calls, sock, ncalls, last, nsocks, call_sock, n, xids, last_out, None)


def test_next_xids_validates_before_any_hip_call():
    for kw in (dict(calls=None), dict(sock=None), dict(last=None), dict(call_sock=None), dict(xids=None)):
        assert nx(**kw) == EINVAL, kw
    assert nx(ncalls=0xFFFFFFFF, n=1) == EINVAL and nx(ncalls=1, n=0xFFFFFFFF) == EINVAL  # no n free values left
    assert nx(ncalls=1 << 32) == EINVAL and nx(n=1 << 32) == EINVAL and nx(nsocks=1 << 32) == EINVAL
    # d_last_out against d_last: equal, overlapping from either side, and just clear of it
    L = FAKE + 2 * FAR
    assert nx(last_out=L) == EINVAL
    assert nx(last_out=L + 12) == EINVAL and nx(last_out=L - 12) == EINVAL
    assert nx(nsocks=1000, last_out=L + 4 * 999) == EINVAL and nx(nsocks=1000, last_out=L - 4 * 999) == EINVAL
    assert nx(last_out=L + 16, xids=FAKE + 2) == EALIGN and nx(last_out=L - 16, xids=FAKE + 2) == EALIGN  # adjacent: legal
    assert nx(calls=FAKE + 4) == EALIGN  # calls: 8
    for kw in (dict(sock=FAKE + FAR + 2), dict(last=L + 2), dict(call_sock=FAKE + 3 * FAR + 2),
               dict(xids=FAKE + 4 * FAR + 2), dict(last_out=FAKE + 5 * FAR + 2)):
        assert nx(**kw) == EALIGN, kw
    # nothing to do: no launch
    assert nx(n=0, nsocks=0, last=None, last_out=None, call_sock=None, xids=None) == 0
    assert nx(n=0, last_out=None, call_sock=None, xids=None) == 0
    assert nx(calls=None, sock=None, ncalls=0, n=0, nsocks=0, last=None, last_out=FAKE, call_sock=None, xids=None) == 0


def pa(calls=FAKE, sock=FAKE + FAR, ncalls=3, new=FAKE + 2 * FAR, new_sock=FAKE + 3 * FAR, n=5,
       merged=FAKE + 4 * FAR, merged_sock=FAKE + 5 * FAR, old_pos=None, new_pos=None):
    return A.lib().xdrg_rpc_socks_pending_add(calls, sock, ncalls, new, new_sock, n, merged, merged_sock, old_pos,
                                              new_pos, None)


def test_pending_add_validates_before_any_hip_call():
    for kw in (dict(calls=None), dict(sock=None), dict(new=None), dict(new_sock=None), dict(merged=None),
               dict(merged_sock=None)):
        assert pa(**kw) == EINVAL, kw
    # d_merged against d_calls and d_new, d_merged_sock against d_sock and d_new_sock: equal and from both sides
    for base, key, width, count in ((FAKE, "merged", 8, 3), (FAKE + 2 * FAR, "merged", 8, 5),
                                    (FAKE + FAR, "merged_sock", 4, 3), (FAKE + 3 * FAR, "merged_sock", 4, 5)):
        assert pa(**{key: base}) == EINVAL, (key, base)
        assert pa(**{key: base + width * (count - 1)}) == EINVAL and pa(**{key: base - width * 7}) == EINVAL
        # adjacent on either side is legal: the next check (alignment of old_pos) is reached
        assert pa(**{key: base + width * count}, old_pos=FAKE + 4) == EALIGN
        assert pa(**{key: base - width * 8}, old_pos=FAKE + 4) == EALIGN
    for kw in (dict(calls=FAKE + 4), dict(new=FAKE + 2 * FAR + 4), dict(merged=FAKE + 4 * FAR + 4),
               dict(old_pos=FAKE + 6 * FAR + 4), dict(new_pos=FAKE + 6 * FAR + 4), dict(sock=FAKE + FAR + 2),
               dict(new_sock=FAKE + 3 * FAR + 2), dict(merged_sock=FAKE + 5 * FAR + 2)):
        assert pa(**kw) == EALIGN, kw
    assert pa(ncalls=1 << 62) == EUNSUPPORTED and pa(n=1 << 62) == EUNSUPPORTED
    assert pa(ncalls=BIG, n=0, new=None, new_sock=None, merged=1 << 50, merged_sock=1 << 52) == EUNSUPPORTED
    assert pa(ncalls=0, n=0, calls=None, sock=None, new=None, new_sock=None, merged=None, merged_sock=None) == 0


def mr(stream=FAKE, length=64, offsets=FAKE + FAR, n=4, msg_row=FAKE + 2 * FAR, row_sock=None, nrows=3,
       calls=FAKE + 3 * FAR, sock=FAKE + 4 * FAR, ncalls=3, hdrs=FAKE + 5 * FAR, call=FAKE + 6 * FAR,
       reply_of=FAKE + 7 * FAR):
    return A.lib().xdrg_rpc_socks_match_replies(stream, length, offsets, n, msg_row, row_sock, nrows, calls, sock,
                                                ncalls, hdrs, call, reply_of, None)


def test_match_replies_validates_before_any_hip_call():
    for kw in (dict(stream=None), dict(offsets=None), dict(msg_row=None), dict(calls=None), dict(sock=None),
               dict(hdrs=None), dict(call=None), dict(reply_of=None)):
        assert mr(**kw) == EINVAL, kw
    for kw in (dict(stream=FAKE + 2), dict(offsets=FAKE + FAR + 4), dict(msg_row=FAKE + 2 * FAR + 2),
               dict(row_sock=FAKE + 2), dict(calls=FAKE + 3 * FAR + 4), dict(sock=FAKE + 4 * FAR + 2),
               dict(hdrs=FAKE + 5 * FAR + 8), dict(call=FAKE + 6 * FAR + 4), dict(reply_of=FAKE + 7 * FAR + 4)):
        assert mr(**kw) == EALIGN, kw
    assert mr(n=BIG * 1) == EUNSUPPORTED and mr(ncalls=1 << 62) == EUNSUPPORTED
    assert mr(n=0, ncalls=0) == 0 and mr(n=0, ncalls=0, stream=None, offsets=None, msg_row=None, calls=None,
                                         sock=None, hdrs=None, call=None, reply_of=None) == 0


def cs(hdrs=FAKE, n=4, reply_of=FAKE + FAR, sock=FAKE + 2 * FAR, ncalls=3, closed=FAKE + 3 * FAR, nsocks=2,
       stats=FAKE + 4 * FAR):
    return A.lib().xdrg_rpc_socks_call_stats(hdrs, n, reply_of, sock, ncalls, closed, nsocks, stats, None)


def test_call_stats_validates_before_any_hip_call():
    for kw in (dict(hdrs=None), dict(reply_of=None), dict(sock=None), dict(closed=None), dict(stats=None)):
        assert cs(**kw) == EINVAL, kw
    for kw in (dict(hdrs=FAKE + 8), dict(reply_of=FAKE + FAR + 4), dict(sock=FAKE + 2 * FAR + 2),
               dict(closed=FAKE + 3 * FAR + 2), dict(stats=FAKE + 4 * FAR + 4)):
        assert cs(**kw) == EALIGN, kw
    assert cs(ncalls=BIG) == EUNSUPPORTED
    assert cs(ncalls=0) == 0 and cs(None, 0, None, None, 0, None, 0, None) == 0


def rt(calls=FAKE, sock=FAKE + FAR, ncalls=3, reply_of=FAKE + 2 * FAR, closed=FAKE + 3 * FAR, nsocks=2,
       kept=FAKE + 4 * FAR, kept_sock=FAKE + 5 * FAR, kept_pos=None, count=FAKE + 6 * FAR, ws=FAKE + 7 * FAR,
       ws_bytes=1 << 40):
    return A.lib().xdrg_rpc_socks_pending_retire(calls, sock, ncalls, reply_of, closed, nsocks, kept, kept_sock,
                                                 kept_pos, count, ws, ws_bytes, None)


def test_pending_retire_validates_before_any_hip_call():
    for kw in (dict(calls=None), dict(sock=None), dict(reply_of=None), dict(closed=None), dict(kept=None),
               dict(kept_sock=None), dict(count=None), dict(ncalls=0, count=None)):
        assert rt(**kw) == EINVAL, kw
    # d_kept against d_calls and d_kept_sock against d_sock: equal, overlapping from either side, adjacent
    for base, key, width in ((FAKE, "kept", 8), (FAKE + FAR, "kept_sock", 4)):
        assert rt(**{key: base}) == EINVAL
        assert rt(**{key: base + 2 * width}) == EINVAL and rt(**{key: base - 2 * width}) == EINVAL
        assert rt(ncalls=1000, **{key: base + 999 * width}) == EINVAL
        assert rt(ncalls=1000, **{key: base - 999 * width}) == EINVAL
        assert rt(**{key: base + 3 * width if width == 8 else base + 16}, ws_bytes=0) == ESPACE
        assert rt(**{key: base - 3 * width if width == 8 else base - 16}, ws_bytes=0) == ESPACE
    for kw in (dict(calls=FAKE + 4), dict(reply_of=FAKE + 2 * FAR + 4), dict(kept=FAKE + 4 * FAR + 4),
               dict(kept_pos=FAKE + 4), dict(count=FAKE + 6 * FAR + 4), dict(ws=FAKE + 7 * FAR + 4),
               dict(sock=FAKE + FAR + 2), dict(closed=FAKE + 3 * FAR + 2), dict(kept_sock=FAKE + 5 * FAR + 2)):
        assert rt(**kw) == EALIGN, kw
    need = A.lib().xdrg_rpc_socks_pending_retire_workspace_size
    assert rt(ws_bytes=need(3) - 1) == ESPACE and rt(ws=None) == ESPACE
    assert rt(ncalls=257, kept=1 << 40, kept_sock=1 << 42, ws_bytes=need(257) - 1) == ESPACE
    assert rt(ncalls=BIG, kept=1 << 50, kept_sock=1 << 52, ws_bytes=need(BIG)) == EUNSUPPORTED
    assert rt(ncalls=BIG - 1, kept=1 << 50, kept_sock=1 << 52, ws_bytes=need(BIG - 1) - 1) == ESPACE
    assert rt(ncalls=1 << 62, kept=1 << 50, kept_sock=1 << 52) == EUNSUPPORTED


def test_workspace_size():
    need, single = A.lib().xdrg_rpc_socks_pending_retire_workspace_size, A.lib().xdrg_rpc_pending_retire_workspace_size
    for n in (0, 1, 256, 257, 1 << 16, SM.TILE * SM.SCAN_LANES + 1, 1 << 31):
        assert need(n) == single(n) and need(n) % 256 == 0 and need(n) >= 8 * ((n + SM.TILE - 1) // SM.TILE)


# ------------------------------------------------ SockCalls and PendingCalls
def test_sockcalls_against_pendingcalls_on_random_tables():
    rng = np.random.default_rng(12)
    for _ in range(200):
        nsocks = int(rng.integers(1, 9))
        nc = int(rng.integers(0, 300))
        pool = rng.integers(0, 40 if rng.random() < 0.5 else 1 << 32, size=(nsocks, nc + 1), dtype=np.int64)
        socks = rng.integers(nsocks, size=nc)
        pairs = np.unique(np.stack([socks, pool[socks, np.arange(nc)]], axis=1), axis=0) if nc else np.zeros((0, 2), np.int64)
        pairs = rng.permutation(pairs)
        socks, xids = pairs[:, 0], pairs[:, 1].astype(np.uint32)
        res = rng.integers(9, size=xids.size)
        last = rng.integers(1 << 32, size=nsocks, dtype=np.int64)
        p = R.SockCalls(socks, xids, res, nsocks, "cpu", last=last)
        tsock, table, perm = KM.sorted_table(socks, xids, res)
        assert p.ncalls == xids.size and p.nsocks == nsocks
        assert np.array_equal(p.calls, table) and np.array_equal(p.socks_numpy(), tsock)
        assert np.array_equal(p.perm.numpy(), perm) and np.array_equal(p.perm.numpy()[p.inv.numpy()], np.arange(xids.size))
        assert np.array_equal(p.last_numpy(), last.astype(np.uint32))
        at = 0
        for g in range(nsocks):
            mine = np.nonzero(socks == g)[0]
            q, want = p.for_sock(g), R.PendingCalls(xids[mine], res[mine], "cpu", last_xid=int(last[g]))
            assert np.array_equal(q.calls, want.calls) and q.last_xid == want.last_xid
            assert np.array_equal(q.inv.numpy(), want.inv.numpy()) and np.array_equal(p.callers_of(g), mine)
            # the table is the concatenation of the single-socket tables, in socket order
            assert np.array_equal(p.calls[at:at + q.ncalls], q.calls)
            assert np.array_equal(p.inv.numpy()[mine], at + q.inv.numpy())
            at += q.ncalls
        r = R.SockCalls.from_device(p.table, p.sock, p.inv, p.last)
        assert np.array_equal(r.perm.numpy(), perm) and r.nsocks == nsocks


def test_sockcalls_refuses_what_is_no_table():
    # two sockets may both have xid 1 outstanding; one socket may not
    assert R.SockCalls([0, 1, 2], [1, 1, 1], 0, device="cpu").ncalls == 3
    with pytest.raises(ValueError):
        R.PendingCalls([1, 1, 1], 0, "cpu")
    with pytest.raises(ValueError):
        R.SockCalls([0, 1, 1], [1, 1, 1], 0, device="cpu")
    with pytest.raises(ValueError):
        R.SockCalls([0, 1, 1], [1, 1, 1 + (1 << 32)], 0, device="cpu")  # the same xid as unsigned
    with pytest.raises(ValueError):
        R.SockCalls([0, 3], [1, 2], 0, nsocks=3, device="cpu")
    e = R.SockCalls([], [], [], nsocks=4, device="cpu")
    assert e.ncalls == 0 and e.nsocks == 4 and e.last_numpy().tolist() == [0] * 4 and e.for_sock(2).ncalls == 0


# ------------------------------------------------------ model consistency
@pytest.mark.parametrize("case", KM.XID_CASES, ids=[c[0] for c in KM.XID_CASES])
@pytest.mark.parametrize("beyond", [False, True])
def test_model_xids_and_merge_against_the_single_socket_models(case, beyond):
    _, socks, xids, res, last, call_sock = case
    if beyond:  # the last two sockets are no sockets: they count from 0
        last = last[:max(last.size - 2, 0)]
    tsock, table, _ = KM.sorted_table(socks, xids, res)
    got, last_out = KM.next_xids(tsock, table, last, call_sock)
    new = np.zeros(call_sock.size, dtype=R.CALL_DTYPE)
    new["xid"], new["res"] = got, np.arange(call_sock.size) % 7
    msock, merged, old_pos, new_pos = KM.pending_add(tsock, table, call_sock, new)
    assert last_out.size == last.size
    seen = 0
    for g in KM.socks_of(tsock, call_sock, np.arange(last.size)):
        lo, hi = KM.run_of(tsock, g)
        a, b = KM.run_of(call_sock, g)
        from_ = int(last[g]) if g < last.size else 0
        want = CS.next_xids_by_search(table["xid"][lo:hi], from_, b - a)
        assert np.array_equal(got[a:b], want), g
        assert np.array_equal(want, CS.next_xids(table["xid"][lo:hi], from_, b - a))
        if g < last.size:
            assert last_out[g] == (want[-1] if b > a else last[g])
        assert not np.isin(want, table["xid"][lo:hi]).any() and np.unique(want).size == want.size
        op, npos = CS.merge_by_search(table["xid"][lo:hi], new["xid"][a:b])
        assert np.array_equal(old_pos[lo:hi], np.asarray(op) + lo + a)
        assert np.array_equal(new_pos[a:b], np.asarray(npos) + lo + a)
        assert (msock[lo + a:hi + b] == g).all()
        seen += (hi - lo) + (b - a)
    assert seen == merged.size
    # the result is a table again: sorted by (sock, xid), no duplicate pair, every entry where its position says
    key = msock.astype(np.uint64) << np.uint64(32) | merged["xid"]
    assert (np.diff(key.astype(object)) > 0).all() if key.size > 1 else True
    assert np.array_equal(merged[old_pos], table) and np.array_equal(merged[new_pos], new)


@pytest.mark.parametrize("name", KM.MATCH_CASES)
def test_model_match_against_reply_model_per_socket(name):
    socks, xids, s, o, rows, row_sock, nrows = KM.match_case(name)
    msock = KM.msg_socks(rows, row_sock, nrows)
    hdrs, call, reply_of = KM.match(s, o, msock, socks, xids)
    action, pcall, preply = KM.match_per_socket(s, o, msock, socks, xids)
    assert np.array_equal(hdrs["action"], action) and np.array_equal(call, pcall) and np.array_equal(reply_of, preply)
    matched = call >= 0
    assert (socks[call[matched]] == msock[matched]).all()  # nobody answers a call of another socket
    if name == "xid1_on_three":
        assert call.tolist() == [-1, -1, 1, -1, 0, 2, -1, -1] and reply_of.tolist() == [4, 2, 5, -1, -1]
        assert (hdrs["action"][~matched] == A.RPCR_UNKNOWN_XID).all()
    if name == "wrong_first":
        assert call.tolist() == [-1, 0, 1, 2] and hdrs["action"][0] == A.RPCR_UNKNOWN_XID
    if name == "row_map":
        assert call.tolist() == [0, 2, 4, -1, -1, 3, 1, -1] and (hdrs["action"][[3, 4, 7]] == A.RPCR_UNKNOWN_XID).all()
    if name.endswith("257"):
        assert np.count_nonzero(matched) > 30 and np.count_nonzero(hdrs["action"] == A.RPCR_UNKNOWN_XID) > 30
        assert (msock == -1).any()


@pytest.mark.parametrize("nc", KM.SIZES)
def test_model_settle_against_settle_model_per_socket(nc):
    tsock, table, nsocks = KM.settle_table(nc)
    rng = np.random.default_rng(nc)
    perm = rng.permutation(nc)  # the caller's order
    socks, xids, res = tsock[perm], table["xid"][perm], table["res"][perm]
    assert np.array_equal(KM.sorted_table(socks, xids, res)[1], table)
    h = np.zeros(1000, dtype=R.HDR_DTYPE)
    h["action"] = np.arange(1000) % 9
    h["w"][:, 1], h["w"][:, 2] = np.arange(1000) % 5, np.arange(1000) % 7
    for cname in (KM.CLOSED_MASKS if nc < 2000 else ("alternating",)):
        closed = KM.closed_mask(cname, nsocks)
        for aname in (KM.ANSWERED if nc < 2000 else ("random",)):
            rt_ = KM.answered(aname, nc)
            reply_of = rt_.view(np.int64)[perm]  # caller c is table entry perm[c]
            kept, kept_sock, kept_pos, count = KM.retire_arrays(tsock, table, rt_, closed)
            ksock, ktable, old_of_new, inv = KM.retire(socks, xids, res, reply_of, closed)
            assert count == len(ktable) and np.array_equal(kept, ktable) and np.array_equal(kept_sock, ksock)
            assert np.array_equal(kept_pos[perm[old_of_new]], inv.astype(np.uint64))
            stats = KM.call_stats(h, reply_of, socks, closed)
            assert np.array_equal(KM.call_stats_arrays(h, rt_, tsock, closed)[perm], stats)
            for g in range(nsocks):
                mine = np.nonzero(socks == g)[0]
                assert np.array_equal(stats[mine], SM.call_stats(h, reply_of[mine], aborted=bool(closed[g])))
                t, old, _ = SM.retire(xids[mine], res[mine], np.zeros(mine.size, np.int64) if closed[g] else reply_of[mine])
                lo, hi = KM.run_of(ksock, g)
                assert np.array_equal(ktable[lo:hi], t) and np.array_equal(np.sort(mine[old]), old_of_new[np.isin(old_of_new, mine)])
            if nc >= 384 and aname == "none":
                want = {"none": nc, "all": 0, "across_tile": nc - 13, "lane0": nc - 1, "lane63": nc - 1}.get(cname)
                assert want is None or count == want
