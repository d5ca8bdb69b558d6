"""TEST INFRASTRUCTURE for tests/test_settle_abi.py and test_gpu_settle.py: a
model of xdrg_rpc_call_stats and xdrg_rpc_pending_retire (include/xdrgpu.h
"Settling a reply batch"), twice.

The literal restatement: rpc_sock::calls_ is a Python dict; recv_msg's erase
at the first reply (xdrpp/msgsock.cc:217-219) is reply_model.match, walked in
message order; the callback's call_result is rpc_call_stat(hdr)
(xdrpp/rpc_msg.cc:69-90, the catch of arpc.h:87-89); abort_all_calls
(msgsock.cc:190-200, arpc.h:60-61) is `aborted`; get_xid after the erases is
call_stream_model.next_xids over the surviving set.

The array form the kernels compute: the keep mask, the kept entries of every
tile, the exclusive scan of the tile counts, a lane's rank from its wave's
ballot.

Calls are named by their position in the caller's `xids`, as
xdrpp_amd.rpc.PendingCalls does, unless a name says `table`.
"""
from __future__ import annotations

import numpy as np

import call_stream_model as CS
import reply_model as RM
from xdrpp_amd import _abi as A
from xdrpp_amd import rpc as R

NO_CALL = np.uint64(A.RPC_NO_CALL)
STAT = A.CALL_STAT_DTYPE
TILE = 256         # kStThreads: the entries of a tile
SCAN_LANES = 1024  # kStScanThreads: the tiles of one round of the scan
WAVE = 64


# ------------------------------------------------------------- call stats
def call_stat(h) -> tuple[int, int]:
    """rpc_call_stat(hdr) for a header after verify_results."""
    a = int(h["action"])
    if a == A.RPCR_OK:
        return A.RPCS_ACCEPT_STAT, 0
    if a == A.RPCR_ACCEPT_STAT:
        return A.RPCS_ACCEPT_STAT, int(h["w"][A.RPC_W_STAT])
    if a == A.RPCR_AUTH_STAT:
        return A.RPCS_AUTH_STAT, int(h["w"][A.RPC_W_WHY])
    if a == A.RPCR_RPCVERS_MISMATCH:
        return A.RPCS_RPCVERS_MISMATCH, 0
    return A.RPCS_GARBAGE_RES, 0


def call_stats(hdrs: np.ndarray, reply_of, aborted: bool = False) -> np.ndarray:
    """What cb receives, per call: reply_of[c] is -1 (or NO_CALL) for a call
    without a reply, a message number, or anything else (GARBAGE_RES)."""
    out = np.zeros(len(reply_of), dtype=STAT)
    for c, i in enumerate(np.asarray(reply_of).astype(np.uint64).tolist()):
        if i == int(NO_CALL):
            out[c] = (A.RPCS_NETWORK_ERROR if aborted else A.RPCS_PENDING, 0)
        elif i < len(hdrs):
            out[c] = call_stat(hdrs[i])
        else:
            out[c] = (A.RPCS_GARBAGE_RES, 0)
    return out


# ----------------------------------------------------- the literal retire
def retire(xids, res, reply_of):
    """calls_ after the erases.  Returns (table CALL_DTYPE [count] sorted by
    xid, old_of_new int64 [count], inv int64 [count]): the survivors are
    renumbered in ascending old caller position, inv[p] is the table position
    of new call p."""
    x = (np.asarray(xids).astype(np.int64) & CS.M32).astype(np.uint32)
    r = np.broadcast_to(np.asarray(res).astype(np.int64) & CS.M32, x.shape).astype(np.uint32)
    calls_ = {int(v): c for c, v in enumerate(x)}
    assert len(calls_) == x.size, "duplicate xid"
    for c, i in enumerate(np.asarray(reply_of).astype(np.int64).tolist()):
        if i != -1:
            del calls_[int(x[c])]  # calls_.erase(i), msgsock.cc:219
    old_of_new = np.array(sorted(calls_.values()), dtype=np.int64)
    new_of_old = {int(c): p for p, c in enumerate(old_of_new)}
    table = np.zeros(len(calls_), dtype=R.CALL_DTYPE)
    inv = np.zeros(len(calls_), dtype=np.int64)
    for t, xid in enumerate(sorted(calls_)):  # std::map order: by xid
        c = calls_[xid]
        table[t] = (xid, r[c])
        inv[new_of_old[c]] = t
    return table, old_of_new, inv


def settle(stream: np.ndarray, offsets: np.ndarray, xids, res, cps: dict, aborted: bool = False,
           stack_limit: int = 0xFFFFFFFF):
    """A reply batch through the dict: (hdrs after the result decode, call,
    reply_of, stats, (table, old_of_new, inv) of calls_ afterwards)."""
    hdrs, call, reply_of = RM.match(stream, offsets, xids)
    r = np.broadcast_to(np.asarray(res), (len(xids),))
    RM.verify_results(stream, hdrs, call, r, cps, stack_limit)
    stats = call_stats(hdrs, reply_of, aborted)
    after = retire(xids, r, np.zeros(len(xids), dtype=np.int64) if aborted else reply_of)  # abort: calls_.clear()
    return hdrs, call, reply_of, stats, after


def next_xids(xids, reply_of, last: int, n: int) -> np.ndarray:
    """get_xid() n times over calls_ after the erases."""
    table, _, _ = retire(xids, 0, reply_of)
    return CS.next_xids(table["xid"], last, n)


# --------------------------------------------------------- the array form
def sorted_table(xids, res):
    """(table CALL_DTYPE sorted by xid, perm: table position -> caller's)."""
    x = (np.asarray(xids).astype(np.int64) & CS.M32).astype(np.uint32)
    r = np.broadcast_to(np.asarray(res).astype(np.int64) & CS.M32, x.shape).astype(np.uint32)
    order = np.argsort(x, kind="stable")
    t = np.zeros(x.size, dtype=R.CALL_DTYPE)
    t["xid"], t["res"] = x[order], r[order]
    return t, order.astype(np.int64)


def popcount_below(mask: np.ndarray) -> np.ndarray:
    """Per lane of every 64-lane wave: the set lanes below it (the ballot and
    a population count under the lane)."""
    w = mask.reshape(-1, WAVE).astype(np.int64)
    return (np.cumsum(w, axis=1) - w).reshape(-1)


def retire_arrays(table: np.ndarray, reply_of_table):
    """The three passes on a sorted table and a reply_of in TABLE order
    (uint64): (kept [count], kept_pos uint64 [ncalls], count, tile_base)."""
    nc = len(table)
    rt = np.asarray(reply_of_table).astype(np.uint64)
    nb = (nc + TILE - 1) // TILE
    keep = np.zeros(nb * TILE, dtype=bool)
    keep[:nc] = rt == NO_CALL
    tile_count = keep.reshape(nb, TILE).sum(axis=1).astype(np.int64)            # pass 1
    tile_base = np.concatenate([[0], np.cumsum(tile_count)])[:nb].astype(np.int64)  # pass 2
    count = int(tile_count.sum())
    wave_count = keep.reshape(nb, TILE // WAVE, WAVE).sum(axis=2).astype(np.int64)
    waves_before = (np.cumsum(wave_count, axis=1) - wave_count)                  # pass 3
    rank = (np.repeat(tile_base, TILE) + np.repeat(waves_before.reshape(-1), WAVE) + popcount_below(keep))[:nc]
    keep = keep[:nc]
    kept = np.zeros(count, dtype=R.CALL_DTYPE)
    kept[rank[keep]] = table[keep]
    kept_pos = np.where(keep, rank.astype(np.uint64), NO_CALL)
    return kept, kept_pos, count, tile_base


def to_table_order(reply_of, perm) -> np.ndarray:
    """A caller-order reply_of (int64, -1 for none) in table order (uint64)."""
    return np.asarray(reply_of).astype(np.int64)[perm].view(np.uint64)


# ------------------------------------------------------------ the cases
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, TILE * SCAN_LANES + 1)
MASKS = ("none", "all", "alternating", "first_of_wave", "kept_first_of_wave", "last_of_tile", "kept_last_of_tile",
         "waves", "random")


def answered_mask(name: str, nc: int) -> np.ndarray:
    """Which TABLE entries a message answers."""
    j = np.arange(nc)
    if name == "none":
        return np.zeros(nc, dtype=bool)
    if name == "all":
        return np.ones(nc, dtype=bool)
    if name == "alternating":
        return j % 2 == 0
    if name == "first_of_wave":
        return j % WAVE == 0
    if name == "kept_first_of_wave":
        return j % WAVE != 0
    if name == "last_of_tile":
        return j % TILE == TILE - 1
    if name == "kept_last_of_tile":
        return j % TILE != TILE - 1
    if name == "waves":  # whole waves answered between kept ones
        return (j // WAVE) % 2 == 1
    assert name == "random"
    return np.random.default_rng(77).random(nc) < 0.5


def answered_values(mask: np.ndarray) -> np.ndarray:
    """A reply_of in table order (uint64) for an answered mask: message
    numbers, and values that are neither NO_CALL nor a message number (they
    count as answered too)."""
    j = np.arange(mask.size, dtype=np.uint64)
    odd = np.array([1 << 40, 0xFFFFFFFFFFFFFFF0, 1 << 63, 0xFFFFFFFF], dtype=np.uint64)  # + at most 6: never NO_CALL
    v = np.where(j % 5 == 3, odd[(j // 5) % 4] + (j % 7), j * 3 % 1000)
    return np.where(mask, v, NO_CALL).astype(np.uint64)


def case_table(nc: int):
    """(xids, res) of nc pending calls in the caller's order: unique xids
    over the whole range, 0 and 2^32 - 1 among them from two entries on."""
    rng = np.random.default_rng(1000 + nc)
    x = np.unique(rng.integers(1 << 32, size=nc + nc // 8 + 8, dtype=np.int64).astype(np.uint32))[:nc]
    if nc >= 2:
        x[0], x[-1] = 0, 0xFFFFFFFF
    assert np.unique(x).size == nc
    return rng.permutation(x), rng.integers(61, size=nc, dtype=np.int64).astype(np.uint32)
