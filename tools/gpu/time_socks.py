"""Times of the many-socket client calls on the table DESIGN.md
7.2.4 and 7.2.5 measured: 1M new calls on 262,144 pending ones, laid out as 1,
4,096 and 262,144 sockets.

    xdrg_rpc_socks_next_xids, _pending_add, _match_replies, _call_stats,
    _pending_retire                       every layout
    xdrg_rpc_next_xids, _pending_add, _match_replies, _call_stats,
    _pending_retire                       the one-socket layout only, the same
                                          arrays: the comparable row.  With
                                          --parent-lib they come from that
                                          library (the parent commit's build),
                                          else from this one
    parent spread                         the single-socket calls' own
                                          run-to-run spread in this session:
                                          the margin the comparison allows

    python tools/gpu/time_socks.py [--n 1048576] [--runs 20] [--parent-lib PATH]

Every result is checked against numpy before anything is timed.  Device
events in one process, after warm-up, median (and min) of --runs runs; a
many-socket call and its single-socket sibling are timed alternately.  One
JSON line per figure."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_verify as TV  # noqa: E402  (timed, report; puts the repository on sys.path)
from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
from xdrpp_amd.marshal import _ptr  # noqa: E402

dev = TV.dev
OLD = 1 << 18  # calls pending before the batch
SINGLE = ("xdrg_rpc_next_xids", "xdrg_rpc_pending_add", "xdrg_rpc_match_replies", "xdrg_rpc_call_stats",
          "xdrg_rpc_pending_retire")


def parent_lib(path):
    """The single-socket entry points of another build of the library."""
    if not path:
        return A.lib(), "this library"
    P = C.CDLL(os.path.abspath(path))
    for name in SINGLE:
        getattr(P, name).argtypes = getattr(A.lib(), name).argtypes
        getattr(P, name).restype = C.c_int
    return P, os.path.basename(path)


def i32(a) -> torch.Tensor:
    return torch.from_numpy((np.asarray(a).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(dev)


def keys(sock, xid) -> np.ndarray:
    return (np.asarray(sock).astype(np.uint64) << np.uint64(32)) | np.asarray(xid).astype(np.uint64)


def replies(xids: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """One 28-byte accepted SUCCESS reply per xid."""
    w = np.zeros((xids.size, 7), dtype=">u4")
    w[:, 0], w[:, 1], w[:, 2] = 0x80000018, xids, 1
    return w.view(np.uint8).reshape(-1), (np.arange(xids.size + 1, dtype=np.uint64) * 28)


def layout(nsocks: int, n: int, runs: int, P, pname: str) -> None:
    rng = np.random.default_rng(3)
    # ---- the table: 262,144 pending calls spread over the sockets, xids near every socket's counter and far from it
    osock = np.sort(rng.integers(nsocks, size=OLD))
    last = np.full(nsocks, 0xFFF00000, dtype=np.int64) if nsocks == 1 else rng.integers(1 << 32, size=nsocks)
    per = max(2 * n // nsocks, 8)
    near = (last[osock] + 1 + rng.integers(0, per, size=OLD)) & 0xFFFFFFFF
    far = rng.integers(1 << 32, size=OLD)
    oxid = np.where(rng.random(OLD) < 0.5, near, far).astype(np.uint32)
    k0, first = np.unique(keys(osock, oxid), return_index=True)
    osock, oxid = osock[first], oxid[first]
    p0 = R.SockCalls(osock, oxid, np.arange(osock.size) % 3, nsocks, dev, last=last)
    nc0 = p0.ncalls
    csock = (np.arange(n, dtype=np.int64) * nsocks) // n  # the batch, in socket order
    d_csock = i32(csock)
    s = torch.cuda.current_stream().cuda_stream
    L = A.lib()

    # ---- next_xids
    xids = torch.empty(n, dtype=torch.int32, device=dev)
    last2 = torch.empty(nsocks, dtype=torch.int32, device=dev)
    R.launch_socks_next_xids(p0, d_csock, xids, last2, s)
    x = xids.cpu().numpy().view(np.uint32)
    # numpy: in its socket's rotated coordinates r = x - last - 1, call k of the run has exactly r - k pending values
    # below it (none is skipped that is free, none is taken that is pending), and is not pending itself
    run_start = np.searchsorted(csock, csock, "left")
    r = (x.astype(np.int64) - last[csock] - 1) & 0xFFFFFFFF
    rot = np.sort(keys(osock, (oxid.astype(np.int64) - last[osock] - 1) & 0xFFFFFFFF))
    below = np.searchsorted(rot, keys(csock, r), "left") - np.searchsorted(rot, keys(csock, 0), "left")
    assert np.array_equal(r - (np.arange(n) - run_start), below) and not np.isin(keys(csock, x), k0).any()
    run_end = np.searchsorted(csock, np.arange(nsocks), "right")
    want_last = np.where(run_end > np.searchsorted(csock, np.arange(nsocks), "left"), x[np.maximum(run_end - 1, 0)],
                         last.astype(np.uint32))
    assert np.array_equal(last2.cpu().numpy().view(np.uint32), want_last)

    # ---- pending_add
    new = (xids.to(torch.int64) & 0xFFFFFFFF) | (1 << 32)  # res = 1
    nc = nc0 + n
    merged, pos = torch.empty(nc, dtype=torch.int64, device=dev), torch.empty(nc, dtype=torch.int64, device=dev)
    msock = torch.empty(nc, dtype=torch.int32, device=dev)
    R.launch_socks_pending_add(p0, new, d_csock, merged, msock, pos[:nc0], pos[nc0:], s)
    tsock0, t0 = p0.socks_numpy(), p0.calls
    allk = np.concatenate([keys(tsock0, t0["xid"]), keys(csock, x)])
    allres = np.concatenate([t0["res"], np.ones(n, np.uint32)])
    order = np.argsort(allk, kind="stable")
    mk = allk[order]
    assert (np.diff(mk.view(np.int64)) != 0).all()
    got = merged.cpu().numpy().view(R.CALL_DTYPE)
    assert np.array_equal(keys(msock.cpu().numpy(), got["xid"]), mk) and np.array_equal(got["res"], allres[order])
    want_pos = np.empty(nc, dtype=np.int64)
    want_pos[order] = np.arange(nc)
    assert np.array_equal(pos.cpu().numpy(), want_pos)
    p = R.SockCalls.from_device(merged, msock, torch.arange(nc, dtype=torch.int64, device=dev), last2)

    # ---- match: every new call answered once, in a shuffled order, on its own socket
    who = rng.permutation(n)
    sb, so = replies(x[who])
    st, od = torch.from_numpy(sb).to(dev), torch.from_numpy(so.view(np.int64)).to(dev)
    rows = i32(csock[who])
    hdrs = R.check_replies(st, od)
    call = torch.empty(n, dtype=torch.int64, device=dev)
    reply_of = torch.empty(nc, dtype=torch.int64, device=dev)
    R.launch_socks_match_replies(st, od, rows, None, nsocks, p, hdrs, call, reply_of, s)
    assert np.array_equal(call.cpu().numpy(), want_pos[nc0:][who])
    want_reply = np.full(nc, -1, dtype=np.int64)
    want_reply[want_pos[nc0:][who]] = np.arange(n)
    assert np.array_equal(reply_of.cpu().numpy(), want_reply)
    assert (R.hdrs_numpy(hdrs)["action"] == A.RPCR_OK).all()

    # ---- stats and retire: half of the table answered, every second socket closed (one socket: open)
    answered = rng.random(nc) < 0.5
    rt_h = np.where(answered, rng.integers(n, size=nc), -1)
    rt = torch.from_numpy(rt_h).to(dev)
    closed_h = (np.arange(nsocks) % 2 == 1).astype(np.int64)
    closed = i32(closed_h)
    stats = torch.empty(nc, dtype=torch.int64, device=dev)
    kept, kept_pos = torch.empty(nc, dtype=torch.int64, device=dev), torch.empty(nc, dtype=torch.int64, device=dev)
    kept_sock = torch.empty(nc, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(L.xdrg_rpc_socks_pending_retire_workspace_size(nc), 16), dtype=torch.uint8, device=dev)
    R.launch_socks_call_stats(hdrs, rt, p, closed, stats, s)
    R.launch_socks_pending_retire(p, rt, closed, kept, kept_sock, kept_pos, count, ws, s)
    tsock = msock.cpu().numpy().astype(np.int64)
    keep = ~answered & (closed_h[tsock] == 0)
    k = int(count.item())
    assert k == int(keep.sum()) and np.array_equal(kept[:k].cpu().numpy(), merged.cpu().numpy()[keep])
    assert np.array_equal(kept_sock[:k].cpu().numpy(), tsock[keep])
    assert np.array_equal(kept_pos.cpu().numpy(), np.where(keep, np.cumsum(keep) - 1, -1))
    ty = R.call_stats_numpy(stats)["type"]
    assert (ty[answered] == A.RPCS_ACCEPT_STAT).all() and (ty[keep] == A.RPCS_PENDING).all()
    assert (ty[~answered & ~keep] == A.RPCS_NETWORK_ERROR).all()

    # ---- the figures
    fns = {
        "next_xids": lambda: R.launch_socks_next_xids(p0, d_csock, xids, last2, s),
        "pending_add": lambda: R.launch_socks_pending_add(p0, new, d_csock, merged, msock, pos[:nc0], pos[nc0:], s),
        "match_replies": lambda: R.launch_socks_match_replies(st, od, rows, None, nsocks, p, hdrs, call, reply_of, s),
        "call_stats": lambda: R.launch_socks_call_stats(hdrs, rt, p, closed, stats, s),
        "pending_retire": lambda: R.launch_socks_pending_retire(p, rt, closed, kept, kept_sock, kept_pos, count, ws, s),
    }
    if nsocks == 1:  # the single-socket siblings on the same arrays, each right after its many-socket call
        x1 = torch.empty(n, dtype=torch.int32, device=dev)
        m1, pos1 = torch.empty(nc, dtype=torch.int64, device=dev), torch.empty(nc, dtype=torch.int64, device=dev)
        call1, reply1 = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(nc, dtype=torch.int64, device=dev)
        stats1, kept1, kpos1 = (torch.empty(nc, dtype=torch.int64, device=dev) for _ in range(3))
        count1 = torch.empty(1, dtype=torch.int64, device=dev)
        hdrs1 = hdrs.clone()
        lx = int(last[0])
        single = {
            "next_xids": lambda: P.xdrg_rpc_next_xids(_ptr(p0.table), nc0, lx, n, _ptr(x1), s),
            "pending_add": lambda: P.xdrg_rpc_pending_add(_ptr(p0.table), nc0, _ptr(new), n, _ptr(m1), _ptr(pos1),
                                                          pos1.data_ptr() + 8 * nc0, s),
            "match_replies": lambda: P.xdrg_rpc_match_replies(_ptr(st), st.numel(), _ptr(od), n, _ptr(p.table), nc,
                                                              _ptr(hdrs1), _ptr(call1), _ptr(reply1), s),
            "call_stats": lambda: P.xdrg_rpc_call_stats(_ptr(hdrs1), n, _ptr(rt), nc, A.RPCS_PENDING, _ptr(stats1), s),
            "pending_retire": lambda: P.xdrg_rpc_pending_retire(_ptr(p.table), nc, _ptr(rt), _ptr(kept1), _ptr(kpos1),
                                                                _ptr(count1), _ptr(ws), ws.numel(), s),
        }
        both = {}
        for name in fns:
            both[name] = fns[name]
            both["single " + name] = single[name]
            both["single again " + name] = single[name]  # the parent against itself: its spread in this session
        assert all(f() == 0 for f in single.values())
        torch.cuda.synchronize()
        assert torch.equal(x1, xids) and torch.equal(m1, merged) and torch.equal(pos1, pos)
        assert torch.equal(call1, call) and torch.equal(reply1, reply_of) and torch.equal(hdrs1, hdrs)
        assert torch.equal(stats1, stats) and torch.equal(kept1[:k], kept[:k]) and torch.equal(kpos1, kept_pos)
        fns = both
    t = TV.timed(fns, runs)
    # bytes moved, the searches not counted: xids out | the entries in, the table, the sockets and the positions out |
    # offsets, two message words, call and reply_of | reply_of, sock, a header line per answered call, the stats |
    # reply_of and sock twice, the kept entries in and out, kept_pos
    nbytes = {"next_xids": 8 * n + 8 * nsocks, "pending_add": 12 * nc + 20 * nc, "match_replies": 8 * n + 8 * n + 8 * n + 16 * nc,
              "call_stats": 20 * nc + 64 * int(answered.sum()), "pending_retire": 32 * nc + 24 * k}
    for name, ms in t.items():
        base = name.split()[-1]
        what = f"socks {nsocks} sockets: {base}" if not name.startswith("single") else \
            f"{name.replace(base, '').strip()} ({pname}): {base}"
        TV.report(what, ms, nbytes[base], entries=nc, calls=n, sockets=nsocks)
    if nsocks == 1:
        for base in nbytes:
            a, b, m = (statistics.median(t[q + base]) for q in ("single ", "single again ", ""))
            print(json.dumps({"what": f"one socket against the single-socket call: {base}", "socks_ms": round(m, 4),
                              "single_ms": round(a, 4), "single_again_ms": round(b, 4),
                              "ratio": round(m / min(a, b), 3),
                              "single_spread": round(abs(a - b) / min(a, b), 3),
                              "single_min_max_ms": [round(min(t["single " + base]), 4), round(max(t["single " + base]), 4)]}),
                  flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--socks", type=int, nargs="*", default=[1, 4096, 262144])
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    P, pname = parent_lib(a.parent_lib)
    for nsocks in a.socks:
        layout(nsocks, a.n, a.runs, P, pname)
