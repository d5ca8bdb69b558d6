"""TEST INFRASTRUCTURE for tests/test_rpc_results_abi.py and
test_gpu_rpc_results.py: the reply batches the asynchronous-client tests run
on, and their expected values from reply_model (no GPU needed to build
them)."""
from __future__ import annotations

import numpy as np

import oracle_bridge as O
import reply_model as RM
import verdict_model as V
from xdrpp_amd import _abi as A
from xdrpp_amd import schemas as S
from xdrpp_amd import workloads as W
from xdrpp_amd.xdr_types import compile_plan

NMSG = 768
# result types of the mixed batch: res -> schema, None for a void result
RES = {0: "rec128", 1: "recvar", 2: "containertest", 3: None}
NO_PLAN_RES = 9  # a result type no call of verify_results serves


def be_words(words) -> np.ndarray:
    return np.array(words, dtype=">u4").view(np.uint8)


def message(body: np.ndarray) -> np.ndarray:
    """message_t: the record mark (marshal.cc:15-31), then the body."""
    return np.concatenate([be_words([body.size | A.MARK_LAST]), body])


def success(xid: int, result: np.ndarray) -> np.ndarray:
    """rpc_success_hdr(xid) + the result (server.h:27-49)."""
    return message(np.concatenate([be_words([xid, 1, 0, 0, 0, 0]), result]))


def error_reply(xid: int, kind: int) -> np.ndarray:
    """The error replies of server.cc:8-67, by kind % 5."""
    kind %= 5
    if kind == 0:
        w = [xid, 1, 0, 0, 0, 1]               # PROG_UNAVAIL
    elif kind == 1:
        w = [xid, 1, 0, 0, 0, 2, 2, 3]         # PROG_MISMATCH low, high
    elif kind == 2:
        w = [xid, 1, 0, 0, 0, 4]               # GARBAGE_ARGS
    elif kind == 3:
        w = [xid, 1, 1, 1, 5]                  # MSG_DENIED, AUTH_ERROR, AUTH_TOOWEAK
    else:
        w = [xid, 1, 1, 0, 2, 2]               # MSG_DENIED, RPC_MISMATCH
    return message(be_words(w))


def stream_of(msgs: list[np.ndarray]):
    stream = np.concatenate(msgs)
    offsets = np.concatenate([[0], np.cumsum([m.size for m in msgs])]).astype(np.uint64)
    return stream, offsets


def unique_xids(rng, count: int) -> np.ndarray:
    x = np.unique(rng.integers(1 << 32, size=2 * count + 16).astype(np.uint32))
    assert x.size >= count
    return rng.permutation(x)[:count].astype(np.uint32)


class MixedBatch:
    """768 messages: success replies with rec128, recvar, containertest and
    void results (every fifth result damaged with verdict_model's recipe, as
    test_gpu_rpc_args.py damages arguments), error replies of every kind
    (every second one with four trailing bytes), replies to unknown xids, a
    result type without a plan, and the calls and malformed messages of
    workloads.rpc_calls.  640 pending calls, some never answered."""

    NCALLS = 640

    def __init__(self):
        rng = np.random.default_rng(23)
        self.cps = {r: None if name is None else compile_plan(S.ALL[name]) for r, name in RES.items()}
        recs = {}
        for r, name in RES.items():
            if name is None:
                continue
            nat, heap = W.GENERATORS[name](NMSG)
            x, offs = O.encode(self.cps[r], nat, NMSG, heap)
            recs[r] = [x[int(offs[i]):int(offs[i + 1])] for i in range(NMSG)]
        fs, fo = W.rpc_calls(512)
        fh = O.rpc_headers(fs, fo, None, client=True)
        foreign = [fs[int(fo[i]):int(fo[i + 1])] for i in np.nonzero(
            (fh["action"] == A.RPCR_NOT_REPLY) | (fh["action"] == A.RPCR_MALFORMED))[0]]
        all_x = unique_xids(rng, self.NCALLS + 128)
        self.xids, unknown = all_x[:self.NCALLS], [int(v) for v in all_x[self.NCALLS:]]
        kinds = list(RES) + [NO_PLAN_RES]
        self.res = np.array([kinds[int(rng.integers(len(kinds)))] for _ in range(self.NCALLS)], dtype=np.uint32)
        msgs, k, nsucc, nerr = [], 0, 0, 0
        for i in range(NMSG):
            if i % 8 == 7:  # no reply to a pending call: a CALL or a malformed message
                msgs.append(foreign[(i // 8) % len(foreign)])
                continue
            if i % 10 == 9:  # "ignoring reply to unknown call"
                msgs.append(success(unknown.pop(), recs[0][i]))
                continue
            c = k
            k += 1
            xid, r = int(self.xids[c]), int(self.res[c])
            if c % 7 == 3:
                m = error_reply(xid, nerr // 2)
                if nerr % 2:  # g.done() must see them
                    m = message(np.concatenate([m[4:], be_words([int(rng.integers(1 << 32))])]))
                nerr += 1
                msgs.append(m)
                continue
            if r in recs:
                result = recs[r][i].copy()
            elif r == NO_PLAN_RES:
                result = be_words(rng.integers(1 << 32, size=int(rng.integers(9))))
            else:
                result = np.zeros(0, dtype=np.uint8)
            if nsucc % 5 == 0:  # damaged: a word replaced, or words cut off / added at the end
                if (nsucc // 5) % 2 == 0 and result.size:
                    V.put_be(result, 4 * int(rng.integers(result.size // 4)), V.damaged_word(rng))
                else:
                    d = int(rng.integers(1, 4)) * (1 if rng.integers(2) or not result.size else -1)
                    result = result[:max(result.size - 4 * -d, 0)] if d < 0 else \
                        np.concatenate([result, be_words(rng.integers(1 << 32, size=d))])
            nsucc += 1
            msgs.append(success(xid, result))
        self.answered = k
        self.stream, self.offsets = stream_of(msgs)
        self.checked = O.rpc_headers(self.stream, self.offsets, None, client=True)
        self.matched, self.call, self.reply_of = RM.match(self.stream, self.offsets, self.xids)
        self.model = self.matched.copy()
        self.verdicts = RM.verify_results(self.stream, self.model, self.call, self.res, self.cps)

    def selected(self, r: int, hdrs=None) -> np.ndarray:
        return RM.selected(self.stream, self.model if hdrs is None else hdrs, self.call, self.res, r)

    def slices(self, idx) -> list[np.ndarray]:
        return RM.slices(self.stream, self.model, idx)


def first_reply_batch(n: int):
    """n success replies with void results where duplicates of an xid sit at
    the message pairs (0, n-1), (63, 64) and (255, 256) that fit, plus one
    triple; the first copy of the pair (0, n-1) is a malformed REPLY (its
    reply_stat is no reply_stat): it still wins.  Pairs that share a message
    (n = 65: 0, 63 and 64) become one group with one xid.  Returns (stream,
    offsets, xids of the pending table, the xid of every message)."""
    rng = np.random.default_rng(100 + n)
    xids = unique_xids(rng, n)
    xid_of = [int(v) for v in xids]
    for a, b in [(a, b) for a, b in ((0, n - 1), (63, 64), (255, 256), (10, 20), (20, 30)) if a < b < n]:
        old, new = xid_of[b], xid_of[a]
        xid_of = [new if x == old else x for x in xid_of]
    msgs = [success(xid_of[i], np.zeros(0, dtype=np.uint8)) for i in range(n)]
    if n > 1:
        msgs[0] = message(be_words([xid_of[0], 1, 7, 0, 0, 0]))  # bad value of stat in reply_body
    stream, offsets = stream_of(msgs)
    return stream, offsets, xids, np.array(xid_of, dtype=np.uint32)
