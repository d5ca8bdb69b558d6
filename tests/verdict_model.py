"""TEST INFRASTRUCTURE for tests/test_gpu_verify.py and test_gpu_rpc_args.py:
the expected verdict of one span -- the restatement oracle's decode of the
slice alone (oracle_bridge.decode(cp, slice, 1, [0, len])), behind the
span rules of include/xdrgpu.h "Per-record decode verdicts" -- and the
fuzz recipe that damages a batch."""
from __future__ import annotations

import numpy as np

import oracle_bridge as O

RECORD_LEVEL = 0xFFFF
PICKS = (0, 1, 2, 3, 4, 16, 17, 400, 401, 0xFFFFFFFF)


def verdict(op: int, code: int) -> int:
    return ((op & 0xFFFF) << 8) | code


def oracle_verdict(cp, xdr: np.ndarray, a: int, b: int, stack_limit: int = 0xFFFFFFFF) -> int:
    """(op << 8) | code of the span [a, b) of xdr, 0 when it decodes."""
    a, b = int(a), int(b)
    if b < a or b > xdr.size or a & 3:  # outside the stream, or a misaligned start: never read
        return verdict(0, 1)
    piece = np.ascontiguousarray(xdr[a:b])
    try:
        O.decode(cp, piece, 1, np.array([0, b - a], dtype=np.uint64), stack_limit)
    except O.OracleError as e:
        return verdict(e.op, e.code)
    return 0


def oracle_verdicts(cp, xdr: np.ndarray, spans: np.ndarray, stack_limit: int = 0xFFFFFFFF) -> np.ndarray:
    return np.array([oracle_verdict(cp, xdr, a, b, stack_limit) for a, b in spans], dtype=np.uint32)


def damaged_word(rng) -> int:
    k = int(rng.integers(len(PICKS) + 1))
    return PICKS[k] if k < len(PICKS) else int(rng.integers(1 << 32))


def put_be(x: np.ndarray, at: int, v: int) -> None:
    x[at:at + 4] = np.frombuffer(int(v).to_bytes(4, "big"), dtype=np.uint8)


def fuzz_batch(xdr: np.ndarray, offsets: np.ndarray, n: int, rng):
    """The first n records of a stream, damaged: record r % 3 == 0 has one
    random word replaced (big-endian), r % 3 == 1 has its end moved by -4k,
    +4k (k in 1..3) or +-1..3 bytes, clamped to [begin, len]; r % 3 == 2 is
    intact.  Returns (stream copy, spans int64 [n, 2])."""
    x = xdr.copy()
    spans = np.stack([offsets[:n], offsets[1:n + 1]], axis=1).astype(np.int64)
    for r in range(n):
        a, b = (int(v) for v in spans[r])
        if r % 3 == 0:
            if b - a >= 4:
                put_be(x, a + 4 * int(rng.integers((b - a) // 4)), damaged_word(rng))
        elif r % 3 == 1:
            m, k = int(rng.integers(4)), int(rng.integers(1, 4))
            spans[r, 1] = min(max(b + (-4 * k, 4 * k, -k, k)[m], a), x.size)
    return x, spans
