"""TEST INFRASTRUCTURE for tests/test_rpc_results_abi.py and
test_gpu_rpc_results.py: a numpy model of xdrg_rpc_match_replies,
xdrg_rpc_verify_results and xdrg_rpc_gather_results (include/xdrgpu.h
"Asynchronous client replies").  Headers come from the restatement
(oracle_bridge.rpc_headers, client mode, no xids), the join is a Python dict
walked in message order (rpc_sock::calls_ and its erase at the first reply,
xdrpp/msgsock.cc:202-232), and result verdicts are the restatement's decode of
the result slice alone (verdict_model.oracle_verdict).  Calls are named by
their position in the caller's `xids`, as xdrpp_amd.rpc.PendingCalls does."""
from __future__ import annotations

import numpy as np

import oracle_bridge as O
import verdict_model as V
from xdrpp_amd import _abi as A

REPLY = 1


def be_word(stream: np.ndarray, at: int) -> int:
    return int.from_bytes(stream[at:at + 4].tobytes(), "big")


def match(stream: np.ndarray, offsets: np.ndarray, xids):
    """(hdrs, call int64 [n], reply_of int64 [ncalls]), -1 for none."""
    hdrs = O.rpc_headers(stream, offsets, None, client=True).copy()
    n = len(offsets) - 1
    table = {int(x) & 0xFFFFFFFF: c for c, x in enumerate(xids)}
    assert len(table) == len(xids), "duplicate xid"
    call = np.full(n, -1, dtype=np.int64)
    reply_of = np.full(len(xids), -1, dtype=np.int64)
    for i in range(n):
        m0, m1 = int(offsets[i]), int(offsets[i + 1])
        if m1 > stream.size or m1 < m0 or m1 - m0 < 12 or m0 & 3:  # no xid + msg_type to read
            continue
        if be_word(stream, m0 + 8) != REPLY:
            continue
        c = table.get(be_word(stream, m0 + 4))
        if c is None or reply_of[c] >= 0:  # unknown call, or erased by its first reply
            hdrs["action"][i] = A.RPCR_UNKNOWN_XID
            continue
        call[i], reply_of[c] = c, i
    return hdrs, call, reply_of


def void_verdict(length: int, a: int, b: int) -> int:
    if b < a or b > length or a & 3:
        return V.verdict(0, A.ERR_OVERFLOW_GET)
    if (b - a) & 3:
        return V.verdict(V.RECORD_LEVEL, A.ERR_SIZE_NOT_MULT4)
    return V.verdict(V.RECORD_LEVEL, A.ERR_TRAILING) if b > a else 0


def verify_results(stream: np.ndarray, hdrs: np.ndarray, call: np.ndarray, res, cps: dict,
                   stack_limit: int = 0xFFFFFFFF) -> np.ndarray:
    """Rewrites hdrs in place; returns the verdicts (uint32 [n]).  cps[res] =
    the result type's compiled plan, None for void; a call whose res is not
    in cps is not handled."""
    verdicts = np.zeros(len(hdrs), dtype=np.uint32)
    for i in range(len(hdrs)):
        c = int(call[i])
        if c < 0 or int(res[c]) not in cps:
            continue
        cp = cps[int(res[c])]
        act = int(hdrs["action"][i])
        a, b = int(hdrs["body_off"][i]), int(hdrs["end"][i])
        v, err = 0, 0
        if act == A.RPCR_OK:
            v = void_verdict(stream.size, a, b) if cp is None else V.oracle_verdict(cp, stream, a, b, stack_limit)
            err = v & 0xFF
        elif act in (A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH):
            v = V.verdict(V.RECORD_LEVEL, A.ERR_TRAILING) if b != a else 0
            err = v & 0xFF
        elif act == A.RPCR_MALFORMED:
            err = int(hdrs["err"][i])
            v = V.verdict(V.RECORD_LEVEL, err)
        if v:
            hdrs["action"][i] = A.RPCR_GARBAGE_RES
            hdrs["err"][i] = err
        verdicts[i] = v
    return verdicts


def selected(stream: np.ndarray, hdrs: np.ndarray, call: np.ndarray, res, want: int) -> np.ndarray:
    """Message indices xdrg_rpc_gather_results selects for result type `want`."""
    r = np.asarray(res, dtype=np.int64)
    ok = (hdrs["action"] == A.RPCR_OK) & (call >= 0)
    ok &= np.where(call >= 0, r[np.clip(call, 0, None)] if len(r) else -1, -1) == want
    ok &= (hdrs["end"] >= hdrs["body_off"]) & (hdrs["end"] <= stream.size)
    return np.nonzero(ok)[0]


def slices(stream: np.ndarray, hdrs: np.ndarray, idx) -> list[np.ndarray]:
    return [stream[int(hdrs["body_off"][i]):int(hdrs["end"][i])] for i in idx]


def gathered(pieces: list[np.ndarray]):
    """(bytes, offsets uint64 [count + 1]) of the pieces back to back."""
    data = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([p.size for p in pieces])]).astype(np.uint64)
    return data, offs
