"""RPC header batches on MI355X through the C ABI.

Host-side mirror of the reference's RPC message handling, batched:

    rpc_server_base::dispatch (xdrpp/server.cc:78-117)
    + srpc_service::process proc switch (srpc.h:121-128)   -> dispatch()
    check_call_hdr (rpc_msg.cc:115-131) + xid test
      of synchronous_client_base::invoke (srpc.h:61-66)     -> check_replies()
    rpc_accepted_error_msg / rpc_prog_mismatch_msg /
      rpc_auth_error_msg / rpc_rpc_mismatch_msg (server.cc:8-67)
                                                            -> error_replies()
    xdr_to_msg(rpc_success_hdr(xid), res) (srpc.h:152)      -> success_reply_type()
                                                               + Marshaler.encode_msgs
    decode_arg per call (server.h:205-214), GARBAGE_ARGS
      for the calls that fail (srpc.h:130-134)              -> verify_args(), gather_args(),
                                                               decode_args()
    rpc_sock::recv_msg (msgsock.cc:202-232): replies in any
      order joined to the pending calls by xid              -> PendingCalls, match_replies()
    the reply callback of asynchronous_client_base::invoke
      (arpc.h:59-90): result + g.done(), GARBAGE_RES for
      the reply that throws                                 -> verify_results(), gather_results(),
                                                               decode_results()
    xdr_to_msg(hdr, a...) of a call (arpc.h:44-59)          -> call_type() + Marshaler.encode_msgs
    asynchronous_client_base::invoke for a batch of calls
      to many procedures (arpc.h:41-59): rpc_sock::get_xid
      (msgsock.h:118-122), xdr_to_msg(hdr, args...), and
      calls_ after send_call (msgsock.cc:227-232)           -> call_batch() (launch_next_xids,
                                                               launch_call_batch, launch_pending_add)
    srpc_service::dispatch's reply (srpc.h:130-153), success
      and error replies in the order srpc_server::run writes
      them (srpc.cc:83-88)                                  -> reply_batch()
    the call_result of invoke's callback, rpc_call_stat(hdr)
      (rpc_msg.cc:69-90), recv_msg's calls_.erase at the
      first reply (msgsock.cc:217-219) and abort_all_calls
      (msgsock.cc:190-200, arpc.h:60-61)                    -> call_stats(), PendingCalls.retire(),
                                                               settle()
    msg_sock::input for many sockets at once (msgsock.cc:
      38-119): whole messages delivered, partial tails kept,
      a framing error closing its own connection only; and
      rpc_sock::recv_msg's test (msgsock.cc:202-225)        -> Receiver, recv_batch(),
                                                               Received.reply_ranges()
    msg_sock::putmsg for many sockets at once (msgsock.cc:
      121-134): message streams in any order routed to their
      connections' write queues; pop_wbytes and output
      (msgsock.cc:137-188) on the host                      -> send_batch(), Sender,
                                                               socks_call_batch_any_order()

Each header decodes to one 64-byte xdrg_rpc_hdr (HDR_DTYPE below).  The
exceptions a client raises for a reply (xdr_call_error with the
rpc_call_stat message, exception.h:25-57, rpc_msg.cc:8-109) come from
raise_for_reply().  Every byte is produced by the HIP kernels of
libxdrgpu.so (xdrpp_amd/csrc/rpc.hip, verify.hip, replies.hip,
reply_batch.hip, call_batch.hip, settle.hip, recv_batch.hip, send_batch.hip).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _abi as A
from .marshal import EncodeResult, Marshaler, Plan, Status, XdrRuntimeError, _EXC, _ptr, _stream
from .xdr_types import Struct, UInt, XdrType

HDR_DTYPE = np.dtype([("xid", "<u4"), ("action", "<u2"), ("err", "u1"), ("mtype", "u1"),
                      ("w", "<u4", (8,)), ("cred_len", "<u4"), ("verf_len", "<u4"),
                      ("body_off", "<u8"), ("end", "<u8")])
assert HDR_DTYPE.itemsize == A.RPC_HDR_BYTES
PROC_DTYPE = np.dtype([("prog", "<u4"), ("vers", "<u4"), ("proc", "<u4"), ("flags", "<u4")])

# ------------------------------------------------------------ call errors
# rpc_errmsg(accept_stat) / rpc_errmsg(auth_stat), xdrpp/rpc_msg.cc:8-64
_ACCEPT_MSG = {0: "RPC executed successfully", 1: "remote hasn't exported program",
               2: "remote can't support version #", 3: "program can't support procedure",
               4: "procedure can't decode params", 5: "RPC system error"}
_AUTH_MSG = {0: "success", 1: "bad credential (seal broken)", 2: "client must begin new session",
             3: "bad verifier (seal broken)", 4: "verifier expired or replayed",
             5: "rejected for security reasons", 6: "bogus response verifier",
             7: "reason unknown", 8: "kerberos generic error", 9: "time of credential expired",
             10: "problem with ticket file", 11: "can't decode authenticator",
             12: "wrong net address in ticket", 13: "no credentials for user",
             14: "problem with context"}


def rpc_errmsg_accept(stat: int) -> str:
    return _ACCEPT_MSG.get(int(stat), "unknown accept_stat error")


def rpc_errmsg_auth(stat: int) -> str:
    return _AUTH_MSG.get(int(stat), "auth_stat error")


class XdrCallError(XdrRuntimeError):
    """xdr_call_error (xdrpp/exception.h:53-57): the server refused the call.
    ``kind`` is the rpc_call_stat type ("accept", "auth", "rpcvers")."""

    def __init__(self, what: str, kind: str, stat: int | None, record: int | None = None):
        super().__init__(what, record)
        self.kind, self.stat = kind, stat


def raise_for_reply(h, record: int | None = None) -> None:
    """What synchronous_client_base::invoke raises for a reply header
    (srpc.h:61-66; check_call_hdr, rpc_msg.cc:115-131); returns for OK."""
    a = int(h["action"])
    if a == A.RPCR_OK:
        return
    if a == A.RPCR_ACCEPT_STAT:
        s = int(h["w"][A.RPC_W_STAT])
        raise XdrCallError(rpc_errmsg_accept(s), "accept", s, record)
    if a == A.RPCR_AUTH_STAT:
        s = int(h["w"][A.RPC_W_WHY])
        raise XdrCallError(rpc_errmsg_auth(s), "auth", s, record)
    if a == A.RPCR_RPCVERS_MISMATCH:  # rpc_call_stat::message, rpc_msg.cc:90-91
        raise XdrCallError("server reported rpcvers field with wrong value", "rpcvers", None, record)
    if a == A.RPCR_NOT_REPLY:
        raise XdrRuntimeError("call received when reply expected", record)
    if a == A.RPCR_BAD_XID:
        raise XdrRuntimeError("synchronous_client: unexpected xid", record)
    code = int(h["err"])
    what = A.lib().xdrg_error_message(code).decode()
    if code == A.ERR_BAD_DISCRIMINANT:  # xdrc's union names (gen_hh.cc:479-481)
        what = ("bad value of mtype in _body_t", "bad value of stat in reply_body",
                "bad value of stat in rejected_reply")[int(h["w"][0])]
    raise _EXC.get(A.lib().xdrg_error_exception(code), XdrRuntimeError)(what, record, None, code)


# ----------------------------------------------------------------- status
def _raise_status(e: A.XdrgError) -> None:
    """The XdrRuntimeError of a status block that holds an error (a batch
    stage's own: an output that is too small); returns for none."""
    if e.code:
        raise XdrRuntimeError(A.lib().xdrg_error_message(e.code).decode(), int(e.record), None, int(e.code))


def _run_status(dev, launch) -> A.XdrgError:
    """launch(status, stream) on the current stream with a fresh Status, then
    the one read of it: raises what it holds, else returns it (total_bytes)."""
    st = Status(dev)
    s = _stream()
    st.init(s)
    launch(st, s)
    e = st.read(s)
    _raise_status(e)
    return e


# --------------------------------------------------------------- registry
def proc_table(services: dict[int, dict[int, list[int]]]) -> np.ndarray:
    """The sorted (prog, vers, proc, flags) table xdrg_rpc_dispatch takes,
    from {prog: {vers: [proc, ...]}} (rpc_server_base::servers_,
    server.h:218-219; an empty proc list registers the interface only)."""
    rows = []
    for prog, vs in services.items():
        for vers, procs in vs.items():
            if procs:
                rows += [(prog, vers, p, 0) for p in sorted(set(procs))]
            else:
                rows.append((prog, vers, 0, A.RPC_PROC_IFACE_ONLY))
    t = np.array(sorted(rows), dtype=np.uint32).reshape(-1, 4)
    if len(t) > A.RPC_MAX_PROCS:
        raise ValueError(f"at most {A.RPC_MAX_PROCS} registered procedures")
    return t


def _check_table(t: np.ndarray) -> None:
    t = np.asarray(t, dtype=np.uint32).reshape(-1, 4)
    keys = [tuple(r[:3]) for r in t]
    if keys != sorted(keys) or len(set(keys)) != len(keys):
        raise ValueError("procedure table must be sorted by (prog, vers, proc) with no duplicates")


# ---------------------------------------------------------------- batches
def hdrs_numpy(hdrs: torch.Tensor) -> np.ndarray:
    """Device xdrg_rpc_hdr array -> numpy structured array (copies)."""
    return hdrs.cpu().numpy().view(HDR_DTYPE).reshape(-1)


def dispatch(stream_bytes: torch.Tensor, offsets: torch.Tensor, procs) -> torch.Tensor:
    """Decode and route every message's rpc_msg header (xdrg_rpc_dispatch).
    offsets: int64 [n+1] message marks (index_messages).  procs: the
    registered procedure table (proc_table()), numpy or a device tensor.
    Returns a uint8 device tensor of n * 64 bytes (xdrg_rpc_hdr records)."""
    dev = stream_bytes.device
    if isinstance(procs, np.ndarray):
        _check_table(procs)
        procs = torch.from_numpy(np.ascontiguousarray(procs, dtype=np.uint32).view(np.int32)).to(dev)
    n = offsets.numel() - 1
    out = torch.empty(max(n, 1) * A.RPC_HDR_BYTES, dtype=torch.uint8, device=dev)
    A.check(A.lib().xdrg_rpc_dispatch(_ptr(stream_bytes), stream_bytes.numel(), _ptr(offsets), n,
                                      _ptr(procs), procs.numel() // 4, _ptr(out), _stream()),
            "xdrg_rpc_dispatch")
    return out[:n * A.RPC_HDR_BYTES]


def check_replies(stream_bytes: torch.Tensor, offsets: torch.Tensor,
                  xids: torch.Tensor | None = None) -> torch.Tensor:
    """Decode every reply header and classify it as the client does
    (xdrg_rpc_check_replies); xids: int32 [n] expected xids or None."""
    dev = stream_bytes.device
    n = offsets.numel() - 1
    out = torch.empty(max(n, 1) * A.RPC_HDR_BYTES, dtype=torch.uint8, device=dev)
    A.check(A.lib().xdrg_rpc_check_replies(_ptr(stream_bytes), stream_bytes.numel(), _ptr(offsets),
                                           n, _ptr(xids), _ptr(out), _stream()),
            "xdrg_rpc_check_replies")
    return out[:n * A.RPC_HDR_BYTES]


class ReplyWriter:
    """Reusable xdrg_rpc_replies launcher (owns status + workspace)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.status = Status(self.device)
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)

    def launch(self, hdrs: torch.Tensor, out: torch.Tensor, offsets: torch.Tensor, stream=None):
        n = hdrs.numel() // A.RPC_HDR_BYTES
        need = A.lib().xdrg_rpc_replies_workspace_size(n)
        if self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        s = _stream() if stream is None else stream
        A.check(A.lib().xdrg_rpc_replies(_ptr(hdrs), n, _ptr(out), out.numel(), _ptr(offsets),
                                         _ptr(self._ws), self._ws.numel(), self.status.ptr, s),
                "xdrg_rpc_replies")

    def __call__(self, hdrs: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        n = hdrs.numel() // A.RPC_HDR_BYTES
        out = torch.empty(max(36 * n, 4), dtype=torch.uint8, device=self.device)
        offs = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        s = _stream()
        self.status.init(s)
        self.launch(hdrs, out, offs, s)
        e = self.status.read(s)
        _raise_status(e)
        return out[:int(e.total_bytes)], offs


def error_replies(hdrs: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The error replies of a dispatched batch as record-marked messages in
    message order (server.cc:8-67); returns (stream, offsets[n+1]) where
    header i's reply is stream[offsets[i]:offsets[i+1]] (empty if none)."""
    return ReplyWriter(hdrs.device)(hdrs)


def success_reply_type(res: XdrType, name: str = "rpc_success_reply") -> Struct:
    """The record xdr_to_msg(rpc_success_hdr(xid), res) marshals
    (server.h:27-49 + the argument pack of marshal.h:252-260): xid, REPLY,
    MSG_ACCEPTED, AUTH_NONE, an empty verf body, SUCCESS, then res.  The
    constant words are staged fields (mtype=1, the rest 0)."""
    return Struct(name, [("xid", UInt), ("mtype", UInt), ("stat", UInt), ("flavor", UInt),
                         ("body", UInt), ("accept", UInt), ("res", res)])


# ------------------------------------------------------- call arguments
def _argplans(plans: dict) -> "C.Array":
    import ctypes as C
    if len(plans) > A.RPC_MAX_ARGPLANS:
        raise ValueError(f"at most {A.RPC_MAX_ARGPLANS} procedures per call (several calls with disjoint tables)")
    arr = (A.XdrgRpcArgplan * max(len(plans), 1))()
    for i, key in enumerate(sorted(plans)):
        prog, vers, proc = key
        arr[i] = A.XdrgRpcArgplan(prog, vers, proc, 0, plans[key].handle)
    return arr


def verify_args(stream_bytes: torch.Tensor, hdrs: torch.Tensor, plans: dict[tuple[int, int, int], Plan],
                stack_limit: int = A.DEFAULT_STACK_LIMIT) -> torch.Tensor:
    """decode_arg (server.h:205-214) for every dispatched call of the batch
    whose (prog, vers, proc) is in `plans`, all procedures in one launch
    (xdrg_rpc_verify_args).  A call whose arguments do not decode becomes
    GARBAGE_ARGS with the error code in `err`, in place in `hdrs`, so
    error_replies() answers it; the others go on.  Returns the verdicts
    (int32 [n]; 0 for every header left untouched).  At most 64 procedures:
    ValueError beyond."""
    arr = _argplans(plans)
    n = hdrs.numel() // A.RPC_HDR_BYTES
    verdicts = torch.zeros(max(n, 1), dtype=torch.int32, device=hdrs.device)
    A.check(A.lib().xdrg_rpc_verify_args(_ptr(stream_bytes), stream_bytes.numel(), _ptr(hdrs), n, arr,
                                         len(plans), stack_limit, _ptr(verdicts), _stream()),
            "xdrg_rpc_verify_args")
    return verdicts[:n]


def _gather(stream_bytes, hdrs, capacity, ws_size, call):
    """What gather_args and gather_results share.  ws_size(n): the C call's
    workspace size; call(n, *tail) makes the C call, `tail` being the arguments
    both end with: out, capacity, offsets, index, count, workspace and its
    size, status, stream."""
    dev = hdrs.device
    n = hdrs.numel() // A.RPC_HDR_BYTES
    # (the pieces gathered are disjoint pieces of the stream: its length holds them)
    cap = stream_bytes.numel() if capacity is None else capacity
    out = torch.empty(max(cap, 4), dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    index = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(ws_size(n), 16), dtype=torch.uint8, device=dev)
    e = _run_status(dev, lambda st, s: call(n, out.data_ptr(), cap, offs.data_ptr(), index.data_ptr(), cnt.data_ptr(),
                                            ws.data_ptr(), ws.numel(), st.ptr, s))
    count = int(cnt.item())
    return out[:int(e.total_bytes)], offs[:count + 1], index[:count]


def gather_args(stream_bytes: torch.Tensor, hdrs: torch.Tensor, key: tuple[int, int, int],
                capacity: int | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The arguments of procedure key = (prog, vers, proc)'s dispatched calls
    as one indexed stream, in message order (xdrg_rpc_gather_args): returns
    (args uint8, offsets int64 [count + 1], index int64 [count] of message
    numbers).  Marshaler.decode(args, count, offsets) decodes them.  One
    sync, for the count and the total.  capacity: bytes of the output
    (default: the stream's length, which always holds them); a smaller one
    raises XdrRuntimeError (XDRG_ERR_OVERFLOW_PUT) with record = the first
    message that does not fit."""
    L = A.lib()
    prog, vers, proc = key
    return _gather(stream_bytes, hdrs, capacity, L.xdrg_rpc_gather_workspace_size, lambda n, *tail: A.check(
        L.xdrg_rpc_gather_args(_ptr(stream_bytes), stream_bytes.numel(), _ptr(hdrs), n, prog, vers, proc, *tail),
        "xdrg_rpc_gather_args"))


def _decode_each(plans: dict, gather, dev, stack_limit: int) -> dict:
    """{key: (index, native, heap)} for every key of `plans`, in order:
    gather(key) gives (bytes, offsets, index), and Marshaler.decode the
    records.  A void plan (None) has native = heap = None."""
    out = {}
    for key in sorted(plans):
        data, offs, index = gather(key)
        if plans[key] is None:
            out[key] = (index, None, None)
        elif index.numel() == 0:  # no entry of this key is left
            out[key] = (index, torch.empty(0, dtype=torch.uint8, device=dev), None)
        else:
            native, heap = Marshaler(plans[key], dev).decode(data, index.numel(), offs, stack_limit)
            out[key] = (index, native, heap)
    return out


def decode_args(stream_bytes: torch.Tensor, hdrs: torch.Tensor, plans: dict[tuple[int, int, int], Plan],
                stack_limit: int = A.DEFAULT_STACK_LIMIT) -> dict:
    """The server's argument step for a dispatched batch: verify_args (the
    calls that fail become GARBAGE_ARGS in `hdrs`), then per procedure
    gather_args and Marshaler.decode of the calls left.  Returns
    {key: (index, native, heap)}: the message numbers, and their decoded
    records in that order."""
    keys = sorted(plans)
    for k0 in range(0, len(keys), A.RPC_MAX_ARGPLANS):
        verify_args(stream_bytes, hdrs, {k: plans[k] for k in keys[k0:k0 + A.RPC_MAX_ARGPLANS]}, stack_limit)
    return _decode_each(plans, lambda key: gather_args(stream_bytes, hdrs, key), hdrs.device, stack_limit)


# ------------------------------------------------------ the reply stream
class _Source:
    """What ResultSource and ArgSource share: the output of one
    Marshaler.encode (xdr, with offsets or fixed_size) and the message of each
    of its entries (index, count, count_cap).  _what: the call and the noun of
    the error messages."""
    _what = ("", "")

    @property
    def cap(self) -> int:
        return self.index.numel() if self.count_cap is None else self.count_cap

    @classmethod
    def _encoded(cls, index: torch.Tensor, xdr, offsets_or_fixed_size) -> tuple:
        """(xdr, offsets, fixed_size) from result_source()'s and arg_source()'s
        last two arguments."""
        if isinstance(xdr, EncodeResult):
            if offsets_or_fixed_size is None:
                offsets_or_fixed_size = xdr.offsets
            xdr = xdr.xdr
        if xdr is None:
            return None, None, 0
        if isinstance(offsets_or_fixed_size, torch.Tensor):
            return xdr, offsets_or_fixed_size, 0
        if offsets_or_fixed_size is None:
            if index.numel() == 0 or xdr.numel() % index.numel():
                raise ValueError("%s: fixed-size %s need their wire size" % cls._what)
            offsets_or_fixed_size = xdr.numel() // index.numel()
        return xdr, None, int(offsets_or_fixed_size)

    def _fields(self) -> tuple:
        """The fields xdrg_rpc_result_src and xdrg_rpc_arg_src start with."""
        if self.xdr is None or self.xdr.numel() == 0:  # no bytes: void results, a procedure without arguments
            if self.cap and self.fixed_size:
                raise ValueError("%s: fixed-size %s without bytes" % self._what)
            return None, None, _ptr(self.index), _ptr(self.count), 0, self.cap, 0
        return (_ptr(self.xdr), _ptr(self.offsets), _ptr(self.index), _ptr(self.count), self.xdr.numel(), self.cap,
                self.fixed_size)


def _src_array(sources, ctype, limit: int, noun: str, extra) -> "C.Array":
    if len(sources) > limit:
        raise ValueError(f"at most {limit} {noun} sources per call")
    arr = (ctype * max(len(sources), 1))()
    for k, r in enumerate(sources):
        arr[k] = ctype(*r._fields(), *extra(r))
    return arr


@dataclass
class ResultSource(_Source):
    """One xdrg_rpc_result_src: the results of one Marshaler.encode and the
    message each of them answers.  index: int64 [count] message numbers
    (gather_args' index).  xdr: the encoded results, None for void results.
    offsets: int64 [count + 1] (a var plan's EncodeResult.offsets), or None
    with fixed_size = the plan's wire size.  count: an int64 [1] device tensor
    read by the kernels (min(count, count_cap) entries are used), or None."""
    index: torch.Tensor
    xdr: torch.Tensor | None = None
    offsets: torch.Tensor | None = None
    fixed_size: int = 0
    count: torch.Tensor | None = None
    count_cap: int | None = None
    _what = ("reply_batch", "results")


def _result_srcs(sources) -> "C.Array":
    return _src_array(sources, A.XdrgRpcResultSrc, A.RPC_MAX_RESULT_SRCS, "result", lambda r: ())


def launch_reply_batch(hdrs: torch.Tensor, sources: list[ResultSource], out: torch.Tensor, offsets: torch.Tensor,
                       unused: torch.Tensor | None, status: Status, ws: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_reply_batch as it is: out uint8, offsets int64 [n + 1], unused
    int64 [1] or None, ws uint8 of xdrg_rpc_reply_batch_workspace_size(n)
    bytes.  `status` is not initialised here.  Kernels only: capturable."""
    n = hdrs.numel() // A.RPC_HDR_BYTES
    A.check(A.lib().xdrg_rpc_reply_batch(_ptr(hdrs), n, _result_srcs(sources), len(sources), _ptr(out), out.numel(),
                                         _ptr(offsets), _ptr(unused), _ptr(ws), ws.numel(), status.ptr,
                                         _stream() if stream is None else stream), "xdrg_rpc_reply_batch")


def result_source(index: torch.Tensor, xdr=None, offsets_or_fixed_size=None) -> ResultSource:
    """A ResultSource from (index, xdr, offsets_or_fixed_size): xdr None for
    void results, a uint8 tensor, or what Marshaler.encode returned; the last
    an int64 offsets tensor, the wire size of a fixed plan, or None (taken
    from the EncodeResult; a fixed plan's size is then bytes / count)."""
    return ResultSource(index, *ResultSource._encoded(index, xdr, offsets_or_fixed_size))


def reply_batch(hdrs: torch.Tensor, results: list, capacity: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The replies of a dispatched batch whose handlers have run, as the one
    stream srpc_server::run writes (srpc.cc:83-88): per message, in message
    order, the success reply of the result that answers it, the error reply
    of its header (error_replies()), or nothing (xdrg_rpc_reply_batch).
    results: a list of (index, xdr, offsets_or_fixed_size) -- see
    result_source() -- or ResultSource; at most 64: ValueError beyond.
    Returns (stream, offsets int64 [n + 1]); reply i is
    stream[offsets[i]:offsets[i + 1]].  One sync, for the total.  capacity:
    bytes of the output (default 36 n + 28 entries + the result bytes, which
    always holds them); a smaller one raises XdrRuntimeError
    (XDRG_ERR_OVERFLOW_PUT) with record = the first message that does not
    fit."""
    srcs = [r if isinstance(r, ResultSource) else result_source(*r) for r in results]
    if len(srcs) > A.RPC_MAX_RESULT_SRCS:
        raise ValueError(f"at most {A.RPC_MAX_RESULT_SRCS} result sources per call")
    dev = hdrs.device
    n = hdrs.numel() // A.RPC_HDR_BYTES
    cap = capacity
    if cap is None:
        cap = 36 * n + sum(28 * r.cap + (0 if r.xdr is None else r.xdr.numel()) for r in srcs)
    out = torch.empty(max(cap, 4), dtype=torch.uint8, device=dev)[:cap]
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(A.lib().xdrg_rpc_reply_batch_workspace_size(n), 16), dtype=torch.uint8, device=dev)
    e = _run_status(dev, lambda st, s: launch_reply_batch(hdrs, srcs, out, offs, None, st, ws, s))
    return out[:int(e.total_bytes)], offs


# ------------------------------------------------ the asynchronous client
CALL_DTYPE = np.dtype([("xid", "<u4"), ("res", "<u4")])
assert CALL_DTYPE.itemsize == A.RPC_CALL_BYTES


def call_type(args: XdrType | None = None, name: str = "rpc_call") -> Struct:
    """The record xdr_to_msg(hdr, a...) marshals for a call (arpc.h:44-59,
    srpc.cc:71-80): the call header's ten words -- xid, mtype = CALL (0),
    rpcvers = 2, prog, vers, proc and two AUTH_NONE opaque_auth with empty
    bodies (flavor 0, length 0) -- as staged fields, then the argument
    record.  args=None: a procedure without arguments."""
    fields = [(f, UInt) for f in ("xid", "mtype", "rpcvers", "prog", "vers", "proc",
                                  "cred_flavor", "cred_len", "verf_flavor", "verf_len")]
    if args is not None:
        fields.append(("args", args))
    return Struct(name, fields)


class _CallTable:
    """What PendingCalls and SockCalls keep: `table` (xdrg_rpc_call records
    int64 [ncalls], sorted), `perm` (table position -> the caller's) and `inv`
    (the caller's -> table position), all on the device."""

    def _from_host(self, order: np.ndarray, xids: np.ndarray, res: np.ndarray, device) -> None:
        """The caller's uint32 xids and res, and the order that sorts them."""
        t = np.empty(order.size, dtype=CALL_DTYPE)
        t["xid"], t["res"] = xids[order], res[order]
        inv = np.empty(order.size, dtype=np.int64)
        inv[order] = np.arange(order.size, dtype=np.int64)
        self.device = torch.device(device)
        self.ncalls = int(order.size)
        self._calls = t  # host copy, sorted
        self.table = torch.from_numpy(t.view(np.int64).copy()).to(self.device)
        self.perm = torch.from_numpy(order.astype(np.int64)).to(self.device)
        self.inv = torch.from_numpy(inv).to(self.device)

    def _from_device(self, table: torch.Tensor, inv: torch.Tensor) -> None:
        self.device = table.device
        self.ncalls = int(table.numel())
        self._calls = None
        self.table, self.inv = table, inv
        self.perm = torch.empty_like(inv)
        self.perm[inv] = torch.arange(self.ncalls, dtype=torch.int64, device=self.device)

    @property
    def calls(self) -> np.ndarray:
        """The sorted table on the host (a device-built one is copied at the
        first use)."""
        if self._calls is None:
            self._calls = self.table.cpu().numpy().view(CALL_DTYPE).reshape(-1).copy()
        return self._calls

    def to_caller(self, call: torch.Tensor) -> torch.Tensor:
        """d_call (table positions, -1 for none) in the caller's positions."""
        if self.ncalls == 0:
            return call
        return torch.where(call >= 0, self.perm[call.clamp(min=0)], call)

    def to_table(self, call: torch.Tensor) -> torch.Tensor:
        if self.ncalls == 0:
            return call
        return torch.where(call >= 0, self.inv[call.clamp(min=0)], call)

    def calls_to_caller(self, t: torch.Tensor) -> torch.Tensor:
        """A tensor with one entry per call (reply_of, stats) from table order
        into the caller's."""
        return t[self.inv] if self.ncalls else t

    def calls_to_table(self, t: torch.Tensor) -> torch.Tensor:
        if self.ncalls == 0:
            return t
        out = torch.empty_like(t)
        out[self.inv] = t
        return out

    def _survivors(self, kept_pos: torch.Tensor, count: torch.Tensor) -> tuple[int, torch.Tensor, torch.Tensor]:
        """The caller's numbering after a retire launch (its d_kept_pos int64
        [ncalls] in TABLE positions and d_count): (k, inv2, old_of_new), the
        survivors renumbered 0..k-1 in ascending old caller position, inv2
        int64 [k] the new table position of new call p, old_of_new int64 [k]
        its old caller position.  One sync, for the count; none for an empty
        table."""
        dev, nc = self.device, self.ncalls
        if nc == 0:
            e = torch.empty(0, dtype=torch.int64, device=dev)
            return 0, e, e.clone()
        pos = kept_pos[self.inv]  # a survivor's new table position, by old caller position
        alive = pos >= 0
        rank = torch.cumsum(alive, 0) - 1
        k = int(count.item())  # the one sync
        # survivor c is new call rank[c]; the retired ones all land on a spare slot k
        slot = torch.empty(k + 1, dtype=torch.int64, device=dev)
        slot.scatter_(0, torch.where(alive, rank, k), torch.arange(nc, dtype=torch.int64, device=dev))
        old_of_new = slot[:k]
        return k, pos[old_of_new], old_of_new


def _as_u32(v, shape=None) -> np.ndarray:
    """Integers of the host or the device as uint32 (mod 2^32), flat or broadcast to `shape`."""
    v = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.int64) & 0xFFFFFFFF
    return (v.reshape(-1) if shape is None else np.broadcast_to(v, shape)).astype(np.uint32)


class PendingCalls(_CallTable):
    """rpc_sock::calls_ (msgsock.h) for a batch: the outstanding calls keyed
    by xid, each with `res`, the number of its result type.  Sorts by xid as
    unsigned (the table xdrg_rpc_match_replies searches), raises ValueError on
    a duplicate xid, and keeps the device table and the permutation, so that
    everything the functions below take and return names a call by its
    position in `xids`.  last_xid: rpc_sock::xid_, the last xid handed out (0
    in a fresh rpc_sock); call_batch() counts on from it."""

    def __init__(self, xids, res, device="cuda", *, last_xid: int = 0):
        x = _as_u32(xids)
        r = _as_u32(res, x.shape)
        order = np.argsort(x, kind="stable")
        xs = x[order]
        if np.any(xs[1:] == xs[:-1]):
            raise ValueError("PendingCalls: duplicate xid")
        self._from_host(order, x, r, device)
        self.last_xid = int(last_xid) & 0xFFFFFFFF

    @classmethod
    def from_device(cls, table: torch.Tensor, inv: torch.Tensor, *, last_xid: int = 0) -> "PendingCalls":
        """A table that is on the device already, without a host sort: `table`
        int64 [ncalls], xdrg_rpc_call records sorted by xid as unsigned with
        no duplicates (xdrg_rpc_pending_add's d_merged; not checked), `inv`
        int64 [ncalls], the table position of the caller's call c (its
        d_old_pos / d_new_pos)."""
        self = cls.__new__(cls)
        self._from_device(table, inv)
        self.last_xid = int(last_xid) & 0xFFFFFFFF
        return self

    def retire(self, reply_of: torch.Tensor) -> tuple["PendingCalls", torch.Tensor]:
        """calls_ after the erases of a reply batch (recv_msg, msgsock.cc:
        217-219; xdrg_rpc_pending_retire).  reply_of: match_replies()'s, in
        the caller's positions; a call is retired iff its entry is not -1.
        Returns (pending2, old_of_new): the surviving calls renumbered
        0..count-1 in ascending old caller position, old_of_new int64 [count]
        = the old caller position of call p of pending2.  pending2 equals
        PendingCalls(the survivors' xids in that order, their res,
        last_xid=self.last_xid) (erasing a call does not touch xid_), built
        without a host sort or a host copy of the table.  One sync, for the
        count."""
        dev, nc = self.device, self.ncalls
        kept = torch.empty(nc, dtype=torch.int64, device=dev)
        kept_pos = torch.empty(nc, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        if nc:  # an empty table: nothing is launched and nothing read
            ws = torch.empty(max(A.lib().xdrg_rpc_pending_retire_workspace_size(nc), 16), dtype=torch.uint8,
                             device=dev)
            launch_pending_retire(self, self.calls_to_table(reply_of), kept, kept_pos, count, ws)
        k, inv2, old_of_new = self._survivors(kept_pos, count)
        return PendingCalls.from_device(kept[:k], inv2, last_xid=self.last_xid), old_of_new


# ------------------------------------------------ the client's call stream
@dataclass
class ArgSource(_Source):
    """One xdrg_rpc_arg_src: the arguments of one procedure's calls, as one
    Marshaler.encode wrote them, and the call position of each.  key: (prog,
    vers, proc).  res: the number of the procedure's result type (what
    PendingCalls keeps per call).  index: int64 [count] call positions.  xdr:
    the encoded arguments, None for a procedure without arguments.  offsets:
    int64 [count + 1] (a var plan's EncodeResult.offsets), or None with
    fixed_size = the plan's wire size.  count: an int64 [1] device tensor read
    by the kernels (min(count, count_cap) entries are used), or None."""
    key: tuple[int, int, int]
    res: int
    index: torch.Tensor
    xdr: torch.Tensor | None = None
    offsets: torch.Tensor | None = None
    fixed_size: int = 0
    count: torch.Tensor | None = None
    count_cap: int | None = None
    _what = ("call_batch", "arguments")


def arg_source(key, res: int, index: torch.Tensor, xdr=None, offsets_or_fixed_size=None) -> ArgSource:
    """An ArgSource from (key, res, index, xdr, offsets_or_fixed_size): xdr
    None for a procedure without arguments, a uint8 tensor, or what
    Marshaler.encode returned; the last an int64 offsets tensor, the wire size
    of a fixed plan, or None (taken from the EncodeResult; a fixed plan's size
    is then bytes / count)."""
    return ArgSource(tuple(int(v) for v in key), int(res), index,
                     *ArgSource._encoded(index, xdr, offsets_or_fixed_size))


def _arg_srcs(sources) -> "C.Array":
    return _src_array(sources, A.XdrgRpcArgSrc, A.RPC_MAX_ARG_SRCS, "argument", lambda r: (*r.key, r.res))


def launch_next_xids(pending: PendingCalls, xids: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_next_xids as it is: xids int32 [n] takes the next n xids after
    pending.last_xid that are not in pending.table.  Kernels only:
    capturable."""
    A.check(A.lib().xdrg_rpc_next_xids(_ptr(pending.table), pending.ncalls, pending.last_xid, xids.numel(),
                                       _ptr(xids), _stream() if stream is None else stream), "xdrg_rpc_next_xids")


def launch_call_batch(xids: torch.Tensor, sources: list[ArgSource], out: torch.Tensor, offsets: torch.Tensor,
                      sent: torch.Tensor | None, counts: torch.Tensor | None, status: Status, ws: torch.Tensor,
                      stream=None) -> None:
    """xdrg_rpc_call_batch as it is: xids int32 [n], out uint8, offsets int64
    [n + 1], sent int64 [n] (xdrg_rpc_call records) or None, counts int64 [2]
    or None, ws uint8 of xdrg_rpc_call_batch_workspace_size(n) bytes.
    `status` is not initialised here.  Kernels only: capturable."""
    A.check(A.lib().xdrg_rpc_call_batch(_ptr(xids), xids.numel(), _arg_srcs(sources), len(sources), _ptr(out),
                                        out.numel(), _ptr(offsets), _ptr(sent), _ptr(counts), _ptr(ws), ws.numel(),
                                        status.ptr, _stream() if stream is None else stream), "xdrg_rpc_call_batch")


def launch_pending_add(pending: PendingCalls, new: torch.Tensor, merged: torch.Tensor,
                       old_pos: torch.Tensor | None, new_pos: torch.Tensor | None, stream=None) -> None:
    """xdrg_rpc_pending_add as it is: new int64 [n] (launch_call_batch's
    sent; every entry is merged, XDRG_RPC_RES_UNSENT ones too), merged int64
    [ncalls + n], old_pos int64 [ncalls] and new_pos int64 [n] in TABLE
    positions, or None.  Kernels only: capturable."""
    A.check(A.lib().xdrg_rpc_pending_add(_ptr(pending.table), pending.ncalls, _ptr(new), new.numel(), _ptr(merged),
                                         _ptr(old_pos), _ptr(new_pos), _stream() if stream is None else stream),
            "xdrg_rpc_pending_add")


def _as_arg_sources(sources: list) -> list[ArgSource]:
    srcs = [r if isinstance(r, ArgSource) else arg_source(*r) for r in sources]
    if len(srcs) > A.RPC_MAX_ARG_SRCS:
        raise ValueError(f"at most {A.RPC_MAX_ARG_SRCS} argument sources per call")
    return srcs


def _call_batch(pending: _CallTable, srcs: list[ArgSource], n: int, capacity: int | None, next_xids, pending_add):
    """What call_batch and socks_call_batch share: next_xids(xids, stream),
    launch_call_batch and pending_add(sent, merged, old_pos, new_pos, stream)
    on one stream, then the one sync.  The two callables launch the table's
    own xid and merge kernels.  Returns (stream, offsets, xids, merged, inv):
    the new table and the table position of every caller's call, old calls
    first."""
    dev, nc = pending.device, pending.ncalls
    cap = capacity
    if cap is None:
        cap = 44 * n + sum(0 if r.xdr is None else r.xdr.numel() for r in srcs)
    out = torch.empty(max(cap, 4), dtype=torch.uint8, device=dev)[:cap]
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    xids = torch.empty(n, dtype=torch.int32, device=dev)
    sent = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    merged = torch.empty(nc + n, dtype=torch.int64, device=dev)
    pos = torch.empty(nc + n, dtype=torch.int64, device=dev)
    old_pos, new_pos = pos[:nc], pos[nc:]
    ws = torch.empty(max(A.lib().xdrg_rpc_call_batch_workspace_size(n), 16), dtype=torch.uint8, device=dev)

    def launch(st, s):
        next_xids(xids, s)
        launch_call_batch(xids, srcs, out, offs, sent, counts, st, ws, s)
        pending_add(sent, merged, old_pos, new_pos, s)
        unsent, unused = counts.tolist()  # the one sync; the status read that follows is ready
        if unsent or unused:
            raise ValueError(f"call_batch: {unsent} call positions without a usable entry, {unused} entries unused")

    e = _run_status(dev, launch)
    # the caller's call c sits where its old table position went; call i where new entry i went
    return out[:int(e.total_bytes)], offs, xids, merged, torch.cat([old_pos[pending.inv], new_pos])


def call_batch(pending: PendingCalls, sources: list, n: int | None = None,
               capacity: int | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, PendingCalls]:
    """asynchronous_client_base::invoke (arpc.h:41-59) for a batch of n calls
    to many procedures: the next n xids after pending.last_xid that are not
    pending (rpc_sock::get_xid), the calls as the one record-marked stream the
    socket would carry, in call order (xdrg_rpc_call_batch), and calls_ after
    the sends (xdrg_rpc_pending_add), all on the device.
    sources: a list of (key, res, index, xdr, offsets_or_fixed_size) -- see
    arg_source() -- or ArgSource, one per procedure; at most 64: ValueError
    beyond.  n: the calls (default: the sources' entries).  Every call
    position 0..n-1 must be named by exactly one usable entry: ValueError for
    a position left unsent or an entry left unused.  Returns (stream, offsets
    int64 [n + 1], xids int32 [n], pending2): call i is
    stream[offsets[i]:offsets[i + 1]] with xid xids[i].  In pending2 the old
    calls keep their caller positions 0..ncalls-1 and call i is ncalls + i; it
    equals PendingCalls(old xids + xids, old res + the sources' res), built
    without a host sort, and its last_xid is the last xid issued.  One sync,
    for the total and the counts.  capacity: bytes of the output (default 44 n
    + the argument bytes, which always holds them); a smaller one raises
    XdrRuntimeError (XDRG_ERR_OVERFLOW_PUT) with record = the first call that
    does not fit."""
    srcs = _as_arg_sources(sources)
    if n is None:
        n = sum(r.cap for r in srcs)
    out, offs, xids, merged, inv = _call_batch(
        pending, srcs, n, capacity, lambda xids, s: launch_next_xids(pending, xids, s),
        lambda sent, merged, old_pos, new_pos, s: launch_pending_add(pending, sent, merged, old_pos, new_pos, s))
    last = int(xids[-1].item()) & 0xFFFFFFFF if n else pending.last_xid
    return out, offs, xids, PendingCalls.from_device(merged, inv, last_xid=last)


def launch_match_replies(stream_bytes: torch.Tensor, offsets: torch.Tensor, pending: PendingCalls,
                         hdrs: torch.Tensor, call: torch.Tensor, reply_of: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_match_replies as it is: `call` int64 [n] and `reply_of` int64
    [ncalls] in TABLE positions (pending.to_caller converts).  Kernels only:
    capturable."""
    n = offsets.numel() - 1
    A.check(A.lib().xdrg_rpc_match_replies(_ptr(stream_bytes), stream_bytes.numel(), _ptr(offsets), n,
                                           _ptr(pending.table), pending.ncalls, _ptr(hdrs), _ptr(call),
                                           _ptr(reply_of), _stream() if stream is None else stream),
            "xdrg_rpc_match_replies")


def _match_t(stream_bytes, offsets, pending: _CallTable, launch):
    """check_replies, then launch(hdrs, call, reply_of), the table's own match
    launch.  Returns (hdrs, call [n], reply_of [ncalls]) in TABLE positions."""
    dev = stream_bytes.device
    n = offsets.numel() - 1
    hdrs = check_replies(stream_bytes, offsets)
    tcall = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    treply = torch.empty(max(pending.ncalls, 1), dtype=torch.int64, device=dev)
    launch(hdrs, tcall, treply)
    return hdrs, tcall[:n], treply[:pending.ncalls]


def _match_replies_t(stream_bytes, offsets, pending: PendingCalls):
    return _match_t(stream_bytes, offsets, pending, lambda hdrs, tcall, treply: launch_match_replies(
        stream_bytes, offsets, pending, hdrs, tcall, treply))


def match_replies(stream_bytes: torch.Tensor, offsets: torch.Tensor,
                  pending: PendingCalls) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """rpc_sock::recv_msg (msgsock.cc:202-232) for every message: runs
    check_replies without xids, then joins the replies to the pending calls.
    Returns (hdrs, call int64 [n], reply_of int64 [ncalls]): call[i] = the
    call message i answers, reply_of[c] = the message that answers call c, -1
    for none.  The first reply to a call wins; every other reply to it, and
    every reply to no pending call, has action RPCR_UNKNOWN_XID."""
    hdrs, tcall, treply = _match_replies_t(stream_bytes, offsets, pending)
    return hdrs, pending.to_caller(tcall), pending.calls_to_caller(treply)


def _res_runs(plans: dict) -> list[list[int]]:
    """The result numbers of `plans` as runs of consecutive numbers, at most
    RPC_MAX_ARGPLANS long: one xdrg_rpc_verify_results call each (a number
    inside a call's range without a plan would be taken for void)."""
    runs: list[list[int]] = []
    for k in sorted(plans):
        if runs and k == runs[-1][-1] + 1 and len(runs[-1]) < A.RPC_MAX_ARGPLANS:
            runs[-1].append(k)
        else:
            runs.append([k])
    return runs


def launch_verify_results(stream_bytes: torch.Tensor, hdrs: torch.Tensor, call: torch.Tensor,
                          pending: PendingCalls, plans: list, res_base: int, stack_limit: int,
                          verdicts: torch.Tensor | None, stream=None) -> None:
    """xdrg_rpc_verify_results as it is: `call` in TABLE positions, plans[k]
    (a Plan, or None for void) serves res == res_base + k."""
    import ctypes as C
    arr = (C.c_void_p * max(len(plans), 1))(*[None if p is None else p.handle for p in plans])
    n = hdrs.numel() // A.RPC_HDR_BYTES
    A.check(A.lib().xdrg_rpc_verify_results(_ptr(stream_bytes), stream_bytes.numel(), _ptr(hdrs), _ptr(call), n,
                                            _ptr(pending.table), pending.ncalls, arr, len(plans), res_base,
                                            stack_limit, _ptr(verdicts), _stream() if stream is None else stream),
            "xdrg_rpc_verify_results")


def _verify_results_t(stream_bytes, hdrs, tcall, pending, plans, stack_limit):
    n = hdrs.numel() // A.RPC_HDR_BYTES
    total = torch.zeros(max(n, 1), dtype=torch.int32, device=hdrs.device)
    for run in _res_runs(plans):
        v = torch.zeros(max(n, 1), dtype=torch.int32, device=hdrs.device)
        launch_verify_results(stream_bytes, hdrs, tcall, pending, [plans[k] for k in run], run[0], stack_limit, v)
        total |= v  # a message is in one call's range
    return total[:n]


def verify_results(stream_bytes: torch.Tensor, hdrs: torch.Tensor, call: torch.Tensor, pending: PendingCalls,
                   plans: dict[int, Plan | None], stack_limit: int = A.DEFAULT_STACK_LIMIT) -> torch.Tensor:
    """The reply callback of arpc.h:59-90 for every matched reply
    (xdrg_rpc_verify_results): plans[res] is the result type's Plan, None for
    a void result.  A reply whose result does not decode, that has bytes
    left after it (g.done()), or whose header threw becomes RPCR_GARBAGE_RES
    with the code in `err`, in place in `hdrs`.  Returns the verdicts (int32
    [n]; 0 for every header left untouched).  `call` is match_replies()'s."""
    return _verify_results_t(stream_bytes, hdrs, pending.to_table(call), pending, plans, stack_limit)


def _gather_results_t(stream_bytes, hdrs, tcall, pending, res, capacity=None):
    L = A.lib()
    return _gather(stream_bytes, hdrs, capacity, L.xdrg_rpc_gather_results_workspace_size, lambda n, *tail: A.check(
        L.xdrg_rpc_gather_results(_ptr(stream_bytes), stream_bytes.numel(), _ptr(hdrs), _ptr(tcall), n,
                                  _ptr(pending.table), pending.ncalls, res, *tail), "xdrg_rpc_gather_results"))


def _decode_matched(stream_bytes, hdrs, tcall, pending: _CallTable, plans, stack_limit) -> dict:
    """The reply step after the match, for either table: verify (the replies
    that fail become GARBAGE_RES in `hdrs`), then per result type gather and
    decode.  `tcall` in TABLE positions."""
    _verify_results_t(stream_bytes, hdrs, tcall, pending, plans, stack_limit)
    return _decode_each(plans, lambda res: _gather_results_t(stream_bytes, hdrs, tcall, pending, res), hdrs.device,
                        stack_limit)


def gather_results(stream_bytes: torch.Tensor, hdrs: torch.Tensor, call: torch.Tensor, pending: PendingCalls,
                   res: int, capacity: int | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The results of type `res` of the matched replies that are RPCR_OK, as
    one indexed stream in message order (xdrg_rpc_gather_results): returns
    (bytes uint8, offsets int64 [count + 1], index int64 [count] of message
    numbers), as gather_args does for a procedure's arguments."""
    return _gather_results_t(stream_bytes, hdrs, pending.to_table(call), pending, res, capacity)


def decode_results(stream_bytes: torch.Tensor, offsets: torch.Tensor, pending: PendingCalls,
                   plans: dict[int, Plan | None], stack_limit: int = A.DEFAULT_STACK_LIMIT):
    """The client's reply step in one call: match_replies, verify_results
    (the replies that fail become GARBAGE_RES), then per result type
    gather_results and Marshaler.decode of the replies left.  Returns (hdrs,
    call, reply_of, {res: (index, native, heap)}); a void result type has
    native = heap = None."""
    hdrs, tcall, treply = _match_replies_t(stream_bytes, offsets, pending)
    out = _decode_matched(stream_bytes, hdrs, tcall, pending, plans, stack_limit)
    return hdrs, pending.to_caller(tcall), pending.calls_to_caller(treply), out


def call_stat_message(h) -> str:
    """rpc_call_stat::message() (rpc_msg.cc:92-112) of the call_result a reply
    header stands for after verify_results (rpc_call_stat(hdr), rpc_msg.cc:
    69-90; the catch of arpc.h:87-89)."""
    a = int(h["action"])
    if a == A.RPCR_OK:
        return rpc_errmsg_accept(0)
    if a == A.RPCR_ACCEPT_STAT:
        return rpc_errmsg_accept(int(h["w"][A.RPC_W_STAT]))
    if a == A.RPCR_AUTH_STAT:
        return rpc_errmsg_auth(int(h["w"][A.RPC_W_WHY]))
    if a == A.RPCR_RPCVERS_MISMATCH:
        return "server reported rpcvers field with wrong value"
    if a in (A.RPCR_GARBAGE_RES, A.RPCR_MALFORMED, A.RPCR_NOT_REPLY):
        return "unable to unmarshal reply value sent by server"
    raise ValueError("no call stands behind this reply (ignoring reply to unknown call)")


# -------------------------------------------------- settling a reply batch
CALL_STAT_DTYPE = A.CALL_STAT_DTYPE


def launch_call_stats(hdrs: torch.Tensor, reply_of: torch.Tensor, stats: torch.Tensor,
                      unanswered: int = A.RPCS_PENDING, stream=None) -> None:
    """xdrg_rpc_call_stats as it is: hdrs after launch_verify_results,
    `reply_of` int64 [ncalls] in TABLE positions (launch_match_replies'),
    stats int64 [ncalls] (xdrg_rpc_call_stat records, table order).  Kernels
    only: capturable."""
    A.check(A.lib().xdrg_rpc_call_stats(_ptr(hdrs), hdrs.numel() // A.RPC_HDR_BYTES, _ptr(reply_of),
                                        reply_of.numel(), unanswered, _ptr(stats),
                                        _stream() if stream is None else stream), "xdrg_rpc_call_stats")


def launch_pending_retire(pending: PendingCalls, reply_of: torch.Tensor, kept: torch.Tensor,
                          kept_pos: torch.Tensor | None, count: torch.Tensor, ws: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_pending_retire as it is: `reply_of` int64 [ncalls] in TABLE
    positions, kept int64 [ncalls] (xdrg_rpc_call records), kept_pos int64
    [ncalls] in TABLE positions or None, count int64 [1], ws uint8 of
    xdrg_rpc_pending_retire_workspace_size(ncalls) bytes.  Kernels only:
    capturable."""
    A.check(A.lib().xdrg_rpc_pending_retire(_ptr(pending.table), pending.ncalls, _ptr(reply_of), _ptr(kept),
                                            _ptr(kept_pos), _ptr(count), _ptr(ws), ws.numel(),
                                            _stream() if stream is None else stream), "xdrg_rpc_pending_retire")


def call_stats(hdrs: torch.Tensor, reply_of: torch.Tensor, pending: PendingCalls,
               aborted: bool = False) -> torch.Tensor:
    """The call_result the callback of asynchronous_client_base::invoke
    receives for every pending call (rpc_call_stat(hdr), rpc_msg.cc:69-90;
    xdrg_rpc_call_stats): an int64 device tensor [ncalls] of
    xdrg_rpc_call_stat records (call_stats_numpy) in the caller's positions.
    hdrs: the batch's headers after verify_results; reply_of:
    match_replies()'s, in the caller's positions.  A call without a reply is
    RPCS_PENDING, or with aborted=True RPCS_NETWORK_ERROR (abort_all_calls,
    msgsock.cc:190-200)."""
    stats = torch.empty(max(pending.ncalls, 1), dtype=torch.int64, device=hdrs.device)[:pending.ncalls]
    if pending.ncalls == 0:
        return stats
    launch_call_stats(hdrs, pending.calls_to_table(reply_of), stats,
                      A.RPCS_NETWORK_ERROR if aborted else A.RPCS_PENDING)
    return pending.calls_to_caller(stats)


def call_stats_numpy(stats: torch.Tensor) -> np.ndarray:
    """Device xdrg_rpc_call_stat array -> numpy structured array (copies)."""
    return stats.cpu().numpy().view(CALL_STAT_DTYPE).reshape(-1)


def call_stat_text(type: int, stat: int = 0) -> str:
    """rpc_call_stat::message() (rpc_msg.cc:92-112) of an xdrg_rpc_call_stat."""
    t = int(type)
    if t == A.RPCS_ACCEPT_STAT:
        return rpc_errmsg_accept(stat)
    if t == A.RPCS_AUTH_STAT:
        return rpc_errmsg_auth(stat)
    if t == A.RPCS_RPCVERS_MISMATCH:
        return "server reported rpcvers field with wrong value"
    if t == A.RPCS_GARBAGE_RES:
        return "unable to unmarshal reply value sent by server"
    if t == A.RPCS_NETWORK_ERROR:
        return "network error when communicating with server"
    if t == A.RPCS_BAD_ALLOC:
        return "insufficient memory to unmarshal result"
    if t == A.RPCS_PENDING:
        raise ValueError("the call is still pending: no rpc_call_stat yet")
    raise ValueError(f"rpc_call_stat: invalid type {t}")


def settle(stream_bytes: torch.Tensor, offsets: torch.Tensor, pending: PendingCalls,
           plans: dict[int, Plan | None], aborted: bool = False, stack_limit: int = A.DEFAULT_STACK_LIMIT):
    """A reply batch settled: decode_results, then call_stats, then
    PendingCalls.retire.  Returns (stats, results, pending2, old_of_new):
    stats as call_stats() gives them, results decode_results' dictionary,
    pending2 the table for the next round.  aborted=True is abort_all_calls
    (msgsock.cc:190-200) after the batch: every call still outstanding is
    RPCS_NETWORK_ERROR, pending2 is the empty table and old_of_new is empty;
    the stats of answered calls are the same either way."""
    hdrs, _, reply_of, results = decode_results(stream_bytes, offsets, pending, plans, stack_limit)
    stats = call_stats(hdrs, reply_of, pending, aborted)
    if aborted:
        e = torch.empty(0, dtype=torch.int64, device=pending.device)
        return stats, results, PendingCalls.from_device(e, e.clone(), last_xid=pending.last_xid), e.clone()
    pending2, old_of_new = pending.retire(reply_of)
    return stats, results, pending2, old_of_new


# ------------------------------------------------------- the receive side
CONN_IN_DTYPE, CONN_DTYPE = A.CONN_IN_DTYPE, A.CONN_DTYPE
CONN_STATE_NAMES = ("OPEN", "FRAGMENT", "TOO_LONG", "BAD_SIZE", "BAD_RPC")


def check_segs(segs: np.ndarray, buf_len: int) -> np.ndarray:
    """A host table of (begin, len) rows as xdrg_rpc_recv_batch wants it:
    begins multiples of 4, segments ascending, disjoint and inside the buffer.
    Raises AbiError (EINVAL) where the host can see a violation; the kernels
    clamp whatever a device table holds."""
    t = np.ascontiguousarray(segs).view(CONN_IN_DTYPE).reshape(-1) if np.asarray(segs).dtype == CONN_IN_DTYPE \
        else np.array([tuple(int(v) for v in r) for r in np.asarray(segs, dtype=np.uint64).reshape(-1, 2)],
                      dtype=CONN_IN_DTYPE)
    b, n = t["begin"].astype(object), t["len"].astype(object)
    ends = b + n
    if (t["begin"] & 3).any() or any(e > buf_len for e in ends) or any(ends[i] > b[i + 1] for i in range(len(t) - 1)):
        raise A.AbiError("xdrg_rpc_recv_batch failed: EINVAL (segments: begin a multiple of 4, ascending, "
                         "disjoint, inside the buffer)")
    return t


def launch_recv_batch(buf: torch.Tensor, segs: torch.Tensor, max_msg_len: int, flags: int, out: torch.Tensor,
                      offsets: torch.Tensor, count: torch.Tensor, conn_of: torch.Tensor, kind: torch.Tensor | None,
                      conns: torch.Tensor, status: Status, ws: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_recv_batch as it is: buf and out uint8, segs int64 [2 nconns]
    (xdrg_rpc_conn_in records), offsets int64 [max_msgs + 1], count int64 [1],
    conn_of int32 [max_msgs], kind uint8 [max_msgs] or None, conns int64
    [4 nconns] (xdrg_rpc_conn records), ws uint8 of
    xdrg_rpc_recv_batch_workspace_size(nconns, buf.numel()) bytes.  `status`
    is not initialised here.  Kernels only: capturable."""
    A.check(A.lib().xdrg_rpc_recv_batch(_ptr(buf), buf.numel(), _ptr(segs), segs.numel() // 2, max_msg_len, flags,
                                        _ptr(out), out.numel(), offsets.data_ptr(), offsets.numel() - 1,
                                        count.data_ptr(), _ptr(conn_of), _ptr(kind), _ptr(conns), _ptr(ws),
                                        ws.numel(), status.ptr, _stream() if stream is None else stream),
            "xdrg_rpc_recv_batch")


def conns_numpy(conns: torch.Tensor) -> np.ndarray:
    """Device xdrg_rpc_conn array -> numpy structured array (copies)."""
    return conns.cpu().numpy().view(CONN_DTYPE).reshape(-1)


@dataclass
class Received:
    """What recv_batch() delivers: `stream` uint8, the whole messages of every
    connection, connections in table order and each connection's messages in
    wire order; `offsets` int64 [count + 1], message k's mark and then the
    end (what dispatch, check_replies, match_replies and Marshaler.decode_msgs
    take); `count`; `conn_of` int32 [count]; `kind` uint8 [count] (0 CALL, 1
    REPLY) or None without rpc_sock; `conns` int64 [4 nconns], the 32-byte
    xdrg_rpc_conn records (conns_numpy())."""
    stream: torch.Tensor
    offsets: torch.Tensor
    count: int
    conn_of: torch.Tensor
    kind: torch.Tensor | None
    conns: torch.Tensor

    def conns_numpy(self) -> np.ndarray:
        return conns_numpy(self.conns)

    def reply_ranges(self, reply_offsets: torch.Tensor) -> np.ndarray:
        """The byte range of a reply stream that belongs to each connection:
        int64 [nconns, 2], row c = (reply_offsets[first[c]], reply_offsets[
        first[c] + msgs[c]]).  reply_batch writes replies in call order and
        the messages here are in connection order, so a connection's replies
        are ONE contiguous range of the reply stream, ready for one writev,
        and the ranges of consecutive connections tile the stream."""
        c = self.conns_numpy()
        ro = reply_offsets.cpu().numpy()
        first = c["first"].astype(np.int64)
        return np.stack([ro[first], ro[first + c["msgs"].astype(np.int64)]], axis=1).astype(np.int64)


def recv_batch(buf: torch.Tensor, segs, max_msg_len: int = A.MSG_SOCK_MAXMSGLEN, rpc_sock: bool = True) -> Received:
    """msg_sock::input for many connections at once (xdrg_rpc_recv_batch;
    msgsock.cc:38-119, with rpc_sock=True also recv_msg's test, :202-225).
    buf: uint8 device tensor holding every connection's received bytes; segs:
    the (begin, len) table, a numpy array (checked on the host: AbiError for a
    misaligned begin or segments that overlap or leave the buffer) or an int64
    device tensor [2 nconns] (clamped by the kernels).  One sync, for the
    totals.  Raises nothing for a connection's framing error: that closes the
    connection (conns_numpy()["state"]) and no other."""
    dev = buf.device
    if not torch.is_tensor(segs):
        t = check_segs(segs, buf.numel())
        segs = torch.from_numpy(t.view(np.int64).copy()).to(dev)
    nconns = segs.numel() // 2
    total = buf.numel()
    max_msgs = total // 4
    out = torch.empty(max(total, 4), dtype=torch.uint8, device=dev)[:total]
    offs = torch.empty(max_msgs + 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    conn_of = torch.empty(max(max_msgs, 1), dtype=torch.int32, device=dev)[:max_msgs]
    kind = torch.empty(max(max_msgs, 1), dtype=torch.uint8, device=dev)[:max_msgs] if rpc_sock else None
    conns = torch.empty(max(4 * nconns, 4), dtype=torch.int64, device=dev)[:4 * nconns]
    ws = torch.empty(max(A.lib().xdrg_rpc_recv_batch_workspace_size(nconns, total), 16), dtype=torch.uint8,
                     device=dev)
    # (no error can come of it with these capacities)
    e = _run_status(dev, lambda st, s: launch_recv_batch(buf, segs, max_msg_len, A.RECV_RPC_SOCK if rpc_sock else 0,
                                                         out, offs, cnt, conn_of, kind, conns, st, ws, s))
    n = int(cnt.item())
    return Received(out[:int(e.total_bytes)], offs[:n + 1], n, conn_of[:n], None if kind is None else kind[:n], conns)


class Receiver:
    """The host's rdpos_ / rdmsg_ (msgsock.h) for many connections: the bytes
    each has received and not yet had framed.  Host code only; the framing is
    recv_batch's.

        rx.feed(conn, data)         # after each readv
        buf, segs = rx.batch()      # pinned uint8 tensor and (begin, len) table; rx.ids[i] = the connection of row i
        got = recv_batch(buf.to("cuda", non_blocking=True), segs)
        rx.advance(got.conns_numpy())
    """

    def __init__(self):
        self._tail: dict = {}    # connection -> bytearray not yet consumed
        self._need: dict = {}    # connection -> bytes its tail must reach before it is sent again
        self.closed: dict = {}   # connection -> xdrg_conn_state it failed with
        self.ids: list = []      # the connection of each row of the last batch()

    def feed(self, conn, data) -> None:
        if conn in self.closed:
            raise ValueError(f"connection {conn!r} is closed ({CONN_STATE_NAMES[self.closed[conn]]})")
        self._tail.setdefault(conn, bytearray()).extend(bytes(data))

    def pending(self, conn) -> int:
        return len(self._tail.get(conn, b""))

    def batch(self, pin: bool | None = None):
        """Every open connection whose tail has at least `need` bytes (and any
        at all), packed at 16-byte-aligned begins in feed order of first
        appearance.  Returns (buf uint8 tensor, pinned where CUDA is there;
        segs numpy CONN_IN_DTYPE); self.ids holds the connection of each row."""
        ids = [c for c, t in self._tail.items() if len(t) and len(t) >= self._need.get(c, 0)]
        segs = np.zeros(len(ids), dtype=CONN_IN_DTYPE)
        at = 0
        for i, c in enumerate(ids):
            segs[i] = (at, len(self._tail[c]))
            at = (at + len(self._tail[c]) + 15) & ~15
        buf = torch.zeros(at, dtype=torch.uint8)
        if torch.cuda.is_available() if pin is None else pin:
            buf = buf.pin_memory()
        view = buf.numpy()
        for i, c in enumerate(ids):
            b = int(segs["begin"][i])
            view[b:b + len(self._tail[c])] = np.frombuffer(self._tail[c], dtype=np.uint8)
        self.ids = ids
        return buf, segs

    def advance(self, conns: np.ndarray) -> None:
        """Take the xdrg_rpc_conn records of the last batch() (row i =
        connection self.ids[i]): drop the consumed bytes, remember need, close
        what failed."""
        if len(conns) != len(self.ids):
            raise ValueError("advance() takes the records of the last batch()")
        for c, r in zip(self.ids, conns):
            if int(r["state"]) != A.CONN_OPEN:
                self.closed[c] = int(r["state"])
                self._tail.pop(c, None)
                self._need.pop(c, None)
                continue
            del self._tail[c][:int(r["consumed"])]
            self._need[c] = int(r["need"])


# --------------------------------- the asynchronous client, many connections
class SockCalls(_CallTable):
    """The calls_ of many rpc_socks in one table (include/xdrgpu.h "The
    asynchronous client over many connections"): every outstanding call is
    keyed by (sock, xid), `table` (xdrg_rpc_call records) and `sock` (int32
    socket numbers) are sorted by that pair, and `last` (int32 [nsocks], on
    the device) holds every socket's xid_ (0 in a fresh rpc_sock).  Two sockets
    may both have xid 1 pending; a duplicate (sock, xid) raises ValueError.  As
    PendingCalls does, it keeps the permutation, so that everything the
    functions below take and return names a call by its position in `xids`;
    verify_results and gather_results take it as they take a PendingCalls.
    `calls` is a cached host copy (the array sorted here, or one download of a
    device-built table), not a fresh read of the device: do not write to it."""

    def __init__(self, socks, xids, res, nsocks: int | None = None, device="cuda", *, last=None):
        as_np = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        x = _as_u32(xids)
        g = np.broadcast_to(as_np(socks).astype(np.int64), x.shape).astype(np.int64)
        r = _as_u32(res, x.shape)
        if nsocks is None:
            nsocks = int(g.max()) + 1 if g.size else (0 if last is None else len(as_np(last).reshape(-1)))
        if g.size and (g.min() < 0 or g.max() >= nsocks):
            raise ValueError("SockCalls: a socket number outside 0..nsocks-1")
        order = np.lexsort((x, g))  # stable; by sock, then by xid as unsigned
        gs, xs = g[order], x[order]
        if np.any((gs[1:] == gs[:-1]) & (xs[1:] == xs[:-1])):
            raise ValueError("SockCalls: duplicate (sock, xid)")
        self._from_host(order, x, r, device)
        self.nsocks = int(nsocks)
        self.sock = torch.from_numpy(gs.astype(np.int32)).to(self.device)
        lv = np.zeros(nsocks, dtype=np.uint32) if last is None else _as_u32(last, (nsocks,))
        self.last = torch.from_numpy(lv.view(np.int32).copy()).to(self.device)

    @classmethod
    def from_device(cls, table: torch.Tensor, sock: torch.Tensor, inv: torch.Tensor,
                    last: torch.Tensor) -> "SockCalls":
        """A table that is on the device already (xdrg_rpc_socks_pending_add's
        d_merged and d_merged_sock, xdrg_rpc_socks_pending_retire's d_kept and
        d_kept_sock; not checked), `inv` int64 [ncalls] the table position of
        the caller's call c, `last` int32 [nsocks]."""
        self = cls.__new__(cls)
        self._from_device(table, inv)
        self.nsocks, self.sock, self.last = int(last.numel()), sock, last
        return self

    def socks_numpy(self) -> np.ndarray:
        """The socket of every table entry, on the host (copies)."""
        return self.sock.cpu().numpy().astype(np.int64)

    def last_numpy(self) -> np.ndarray:
        return self.last.cpu().numpy().view(np.uint32).copy()

    def for_sock(self, g: int, device=None) -> PendingCalls:
        """Socket g's rpc_sock as a PendingCalls: its calls in ascending
        caller position, its xid_ as last_xid.  Copies to the host."""
        sk, perm, c = self.socks_numpy(), self.perm.cpu().numpy(), self.calls
        mine = np.nonzero(sk == g)[0]
        by_caller = mine[np.argsort(perm[mine], kind="stable")]
        lx = int(self.last_numpy()[g]) if 0 <= g < self.nsocks else 0
        return PendingCalls(c["xid"][by_caller], c["res"][by_caller], self.device if device is None else device,
                            last_xid=lx)

    def callers_of(self, g: int) -> np.ndarray:
        """The caller positions of socket g's calls, ascending: call p of
        for_sock(g) is call callers_of(g)[p] here."""
        sk, perm = self.socks_numpy(), self.perm.cpu().numpy()
        return np.sort(perm[sk == g])


def launch_socks_next_xids(pending: SockCalls, call_sock: torch.Tensor, xids: torch.Tensor,
                           last_out: torch.Tensor | None, stream=None) -> None:
    """xdrg_rpc_socks_next_xids as it is: call_sock int32 [n] non-decreasing,
    xids int32 [n], last_out int32 [nsocks] (not pending.last) or None.
    Kernels only: capturable."""
    A.check(A.lib().xdrg_rpc_socks_next_xids(_ptr(pending.table), _ptr(pending.sock), pending.ncalls,
                                             _ptr(pending.last), pending.nsocks, _ptr(call_sock), xids.numel(),
                                             _ptr(xids), _ptr(last_out), _stream() if stream is None else stream),
            "xdrg_rpc_socks_next_xids")


def launch_socks_pending_add(pending: SockCalls, new: torch.Tensor, new_sock: torch.Tensor, merged: torch.Tensor,
                             merged_sock: torch.Tensor, old_pos: torch.Tensor | None, new_pos: torch.Tensor | None,
                             stream=None) -> None:
    """xdrg_rpc_socks_pending_add as it is: new int64 [n] (launch_call_batch's
    sent), new_sock int32 [n], merged int64 and merged_sock int32 [ncalls +
    n], old_pos int64 [ncalls] and new_pos int64 [n] in TABLE positions, or
    None.  Kernels only: capturable."""
    A.check(A.lib().xdrg_rpc_socks_pending_add(_ptr(pending.table), _ptr(pending.sock), pending.ncalls, _ptr(new),
                                               _ptr(new_sock), new.numel(), _ptr(merged), _ptr(merged_sock),
                                               _ptr(old_pos), _ptr(new_pos),
                                               _stream() if stream is None else stream),
            "xdrg_rpc_socks_pending_add")


def launch_socks_match_replies(stream_bytes: torch.Tensor, offsets: torch.Tensor, msg_row: torch.Tensor,
                               row_sock: torch.Tensor | None, nrows: int, pending: SockCalls, hdrs: torch.Tensor,
                               call: torch.Tensor, reply_of: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_socks_match_replies as it is: msg_row int32 [n] (recv_batch's
    conn_of), row_sock int32 [nrows] or None (a row is its socket), `call`
    int64 [n] and `reply_of` int64 [ncalls] in TABLE positions.  Kernels only:
    capturable."""
    n = offsets.numel() - 1
    A.check(A.lib().xdrg_rpc_socks_match_replies(_ptr(stream_bytes), stream_bytes.numel(), _ptr(offsets), n,
                                                 _ptr(msg_row), _ptr(row_sock), nrows, _ptr(pending.table),
                                                 _ptr(pending.sock), pending.ncalls, _ptr(hdrs), _ptr(call),
                                                 _ptr(reply_of), _stream() if stream is None else stream),
            "xdrg_rpc_socks_match_replies")


def launch_socks_call_stats(hdrs: torch.Tensor, reply_of: torch.Tensor, pending: SockCalls, closed: torch.Tensor,
                            stats: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_socks_call_stats as it is: `reply_of` int64 [ncalls] in TABLE
    positions, closed int32 [nsocks], stats int64 [ncalls] (table order).
    Kernels only: capturable."""
    A.check(A.lib().xdrg_rpc_socks_call_stats(_ptr(hdrs), hdrs.numel() // A.RPC_HDR_BYTES, _ptr(reply_of),
                                              _ptr(pending.sock), pending.ncalls, _ptr(closed), closed.numel(),
                                              _ptr(stats), _stream() if stream is None else stream),
            "xdrg_rpc_socks_call_stats")


def launch_socks_pending_retire(pending: SockCalls, reply_of: torch.Tensor, closed: torch.Tensor,
                                kept: torch.Tensor, kept_sock: torch.Tensor, kept_pos: torch.Tensor | None,
                                count: torch.Tensor, ws: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_socks_pending_retire as it is: `reply_of` int64 [ncalls] in
    TABLE positions, closed int32 [nsocks], kept int64 and kept_sock int32
    [ncalls], kept_pos int64 [ncalls] or None, count int64 [1], ws uint8 of
    xdrg_rpc_socks_pending_retire_workspace_size(ncalls) bytes.  Kernels only:
    capturable."""
    A.check(A.lib().xdrg_rpc_socks_pending_retire(_ptr(pending.table), _ptr(pending.sock), pending.ncalls,
                                                  _ptr(reply_of), _ptr(closed), closed.numel(), _ptr(kept),
                                                  _ptr(kept_sock), _ptr(kept_pos), _ptr(count), _ptr(ws), ws.numel(),
                                                  _stream() if stream is None else stream),
            "xdrg_rpc_socks_pending_retire")


def _sock_tensor(socks, n: int, dev) -> torch.Tensor:
    t = socks if isinstance(socks, torch.Tensor) else torch.from_numpy(np.asarray(socks).astype(np.int64))
    t = t.reshape(-1).to(device=dev, dtype=torch.int32)
    if t.numel() != n:
        raise ValueError(f"one socket number per call: {t.numel()} for {n} calls")
    return t.contiguous()


def socks_call_batch(pending: SockCalls, socks, sources: list, capacity: int | None = None):
    """call_batch() for a batch whose calls go to many connections: socks[i] is
    call position i's socket, non-decreasing (a batch not in socket order
    raises ValueError).  Every socket counts on from its own xid_ over its own
    calls_ (xdrg_rpc_socks_next_xids), the stream is xdrg_rpc_call_batch's, and
    every calls_ takes its sends (xdrg_rpc_socks_pending_add).  Returns
    (stream, offsets int64 [n + 1], xids int32 [n], pending2, ranges): ranges
    int64 numpy [nsocks, 2], socket g's bytes of the stream (one writev per
    connection; the ranges tile the stream).  In pending2 the old calls keep
    their caller positions and call i is ncalls + i.  Errors as call_batch."""
    srcs = _as_arg_sources(sources)
    dev = pending.device
    n = len(socks) if not isinstance(socks, torch.Tensor) else socks.numel()
    call_sock = _sock_tensor(socks, n, dev)
    merged_sock = torch.empty(pending.ncalls + n, dtype=torch.int32, device=dev)
    last2 = torch.empty_like(pending.last)
    # run ends of every socket in the batch, for the ranges (and the order check)
    ends = torch.searchsorted(call_sock.to(torch.int64),
                              torch.arange(pending.nsocks, dtype=torch.int64, device=dev), right=True)
    ordered = bool((call_sock[1:] >= call_sock[:-1]).all().item()) if n > 1 else True
    if not ordered or (n and (int(call_sock[0].item()) < 0 or int(call_sock[-1].item()) >= pending.nsocks)):
        raise ValueError("socks_call_batch: the calls must be in socket order, sockets 0..nsocks-1")
    out, offs, xids, merged, inv = _call_batch(
        pending, srcs, n, capacity, lambda xids, s: launch_socks_next_xids(pending, call_sock, xids, last2, s),
        lambda sent, merged, old_pos, new_pos, s: launch_socks_pending_add(pending, sent, call_sock, merged,
                                                                           merged_sock, old_pos, new_pos, s))
    pending2 = SockCalls.from_device(merged, merged_sock, inv, last2)
    eb = offs[ends].cpu().numpy().astype(np.int64)
    ranges = np.stack([np.concatenate([[0], eb[:-1]]) if eb.size else eb, eb], axis=1).astype(np.int64)
    return out, offs, xids, pending2, ranges


def _row_sock(ids, dev) -> torch.Tensor | None:
    if ids is None:
        return None
    t = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.asarray(list(ids)).astype(np.int64))
    return t.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()


def _socks_match_t(stream_bytes, offsets, rows, pending, ids):
    row_sock = _row_sock(ids, stream_bytes.device)
    nrows = pending.nsocks if row_sock is None else row_sock.numel()
    rows = rows.to(torch.int32).contiguous()
    return _match_t(stream_bytes, offsets, pending, lambda hdrs, tcall, treply: launch_socks_match_replies(
        stream_bytes, offsets, rows, row_sock, nrows, pending, hdrs, tcall, treply))


def socks_match_replies(stream_bytes: torch.Tensor, offsets: torch.Tensor, rows: torch.Tensor, pending: SockCalls,
                        ids=None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """match_replies() with every reply looked up in the calls_ of the socket
    it arrived on (xdrg_rpc_socks_match_replies).  rows: int32 [n], the row of
    every message (recv_batch's conn_of); ids: the socket number of every row
    (Receiver.ids when the connections are named by their socket numbers), or
    None when a row is its socket.  A reply whose xid is pending on another
    socket only is RPCR_UNKNOWN_XID.  Returns (hdrs, call, reply_of) in the
    caller's positions."""
    hdrs, tcall, treply = _socks_match_t(stream_bytes, offsets, rows, pending, ids)
    return hdrs, pending.to_caller(tcall), pending.calls_to_caller(treply)


def closed_socks(received: Received, ids, nsocks: int, also: torch.Tensor | None = None) -> torch.Tensor:
    """The `closed` tensor (int32 [nsocks], on the device) after a recv_batch:
    socket ids[row] is closed when its row's state is not CONN_OPEN, i.e.
    msg_sock::input or rpc_sock::recv_msg would have closed the connection and
    abort_all_calls run.  also: an earlier closed tensor, kept.  Torch ops
    only, no sync."""
    dev = received.conns.device
    state = received.conns.view(-1, 4)[:, 3] >> 32  # xdrg_rpc_conn.state: the high half of the last word
    closed = torch.zeros(nsocks, dtype=torch.int32, device=dev)
    row_sock = _row_sock(ids, dev)
    if row_sock is not None and row_sock.numel():
        ok = (row_sock >= 0) & (row_sock < nsocks)
        closed.scatter_reduce_(0, row_sock.clamp(0, max(nsocks - 1, 0)).to(torch.int64),
                               ((state != A.CONN_OPEN) & ok).to(torch.int32), reduce="amax")
    if also is not None:
        closed = torch.maximum(closed, (also.to(dev) != 0).to(torch.int32))
    return closed


def socks_settle(received, pending: SockCalls, plans: dict[int, Plan | None], closed: torch.Tensor, ids=None,
                 stack_limit: int = A.DEFAULT_STACK_LIMIT):
    """settle() for many connections.  received: a Received, or (stream,
    offsets, rows); ids as in socks_match_replies; closed: int32 [nsocks]
    (closed_socks()).  Returns (stats, results, pending2, old_of_new): stats
    in the caller's positions -- a call without a reply is RPCS_NETWORK_ERROR
    on a closed socket and RPCS_PENDING on an open one --, results as
    decode_results gives them, pending2 every calls_ for the next round (the
    answered calls and those of closed sockets retired, `last` unchanged),
    old_of_new int64 [count] the old caller position of call p of pending2."""
    if isinstance(received, Received):
        stream_bytes, offsets, rows = received.stream, received.offsets, received.conn_of
    else:
        stream_bytes, offsets, rows = received
    dev, nc = pending.device, pending.ncalls
    hdrs, tcall, treply = _socks_match_t(stream_bytes, offsets, rows, pending, ids)
    results = _decode_matched(stream_bytes, hdrs, tcall, pending, plans, stack_limit)
    closed = closed.to(device=dev, dtype=torch.int32).contiguous()
    count = torch.empty(1, dtype=torch.int64, device=dev)
    stats = torch.empty(max(nc, 1), dtype=torch.int64, device=dev)[:nc]
    kept = torch.empty(max(nc, 1), dtype=torch.int64, device=dev)[:nc]
    kept_sock = torch.empty(max(nc, 1), dtype=torch.int32, device=dev)[:nc]
    kept_pos = torch.empty(max(nc, 1), dtype=torch.int64, device=dev)[:nc]
    ws = torch.empty(max(A.lib().xdrg_rpc_socks_pending_retire_workspace_size(nc), 16), dtype=torch.uint8, device=dev)
    launch_socks_call_stats(hdrs, treply, pending, closed, stats)
    launch_socks_pending_retire(pending, treply, closed, kept, kept_sock, kept_pos, count, ws)
    k, inv2, old_of_new = pending._survivors(kept_pos, count)
    pending2 = SockCalls.from_device(kept[:k], kept_sock[:k], inv2, pending.last)
    return pending.calls_to_caller(stats), results, pending2, old_of_new


def socks_call_batch_any_order(pending: SockCalls, socks, sources: list, capacity: int | None = None):
    """socks_call_batch() for calls in application order: socks[i] is call i's
    socket, in any order.  The calls are brought into socket order by a stable
    sort (calls to one socket keep their order, so each rpc_sock hands out its
    xids in the order the application called), every ArgSource.index is
    renumbered, and socks_call_batch does the rest.  Returns (stream, offsets,
    xids, pending2, ranges, order): stream, offsets and ranges as
    socks_call_batch returns them, in socket order, message p of the stream
    being call order[p] (int64 [n]); xids int32 [n] and the caller positions
    of pending2 (call i is ncalls + i) in the application's order.  A socket
    number outside 0..nsocks-1 raises ValueError.  (A client with ONE xid
    space over many connections needs none of this: call_batch() in caller
    order, then send_batch() with the stream, its offsets and conn = socks.)"""
    import dataclasses
    srcs = _as_arg_sources(sources)
    dev = pending.device
    n = len(socks) if not isinstance(socks, torch.Tensor) else socks.numel()
    call_sock = _sock_tensor(socks, n, dev)
    order = torch.sort(call_sock, stable=True).indices
    inv = torch.empty_like(order)
    inv[order] = torch.arange(n, dtype=torch.int64, device=dev)

    def renumber(index: torch.Tensor) -> torch.Tensor:
        ok = (index >= 0) & (index < n)  # an index that names no call stays what it is
        return torch.where(ok, inv[index.clamp(0, max(n - 1, 0))], index) if n else index

    srcs = [dataclasses.replace(r, index=renumber(r.index.to(dev))) for r in srcs]
    out, offs, xids, p2, ranges = socks_call_batch(pending, call_sock[order], srcs, capacity)
    nc = pending.ncalls
    pending2 = SockCalls.from_device(p2.table, p2.sock, torch.cat([p2.inv[:nc], p2.inv[nc:][inv]]), p2.last)
    return out, offs, xids[inv], pending2, ranges, order


# ----------------------------------------------------------- the send side
WQUEUE_DTYPE = A.WQUEUE_DTYPE
SEND_OUTCOME_NAMES = {A.SEND_DROPPED: "DROPPED", A.SEND_EMPTY: "EMPTY", A.SEND_UNUSABLE: "UNUSABLE"}


@dataclass
class SendSource:
    """One xdrg_rpc_send_src: a stream of record-marked messages (reply_batch's,
    call_batch's, recv_batch's), offsets int64 [count + 1], and the connection
    of every entry: conn an int32 [count] device tensor, or an int for a
    stream that goes to one connection.  count: an int64 [1] device tensor
    read by the kernels (min(count, count_cap) entries are used), or None."""
    stream: torch.Tensor
    offsets: torch.Tensor
    conn: torch.Tensor | int
    count: torch.Tensor | None = None
    count_cap: int | None = None

    @property
    def cap(self) -> int:
        return max(self.offsets.numel() - 1, 0) if self.count_cap is None else self.count_cap


def send_source(stream: torch.Tensor, offsets: torch.Tensor, conn) -> SendSource:
    """A SendSource from (stream, offsets, conn): conn an int, or one
    connection number per entry (a tensor, an array, a list)."""
    if isinstance(conn, (int, np.integer)):
        return SendSource(stream, offsets, int(conn))
    return SendSource(stream, offsets, _sock_tensor(conn, max(offsets.numel() - 1, 0), stream.device))


def _send_srcs(sources) -> "C.Array":
    if len(sources) > A.RPC_MAX_SEND_SRCS:
        raise ValueError(f"at most {A.RPC_MAX_SEND_SRCS} message streams per call")
    arr = (A.XdrgRpcSendSrc * max(len(sources), 1))()
    for k, r in enumerate(sources):
        one = not isinstance(r.conn, torch.Tensor)
        arr[k] = A.XdrgRpcSendSrc(_ptr(r.stream), _ptr(r.offsets), None if one else _ptr(r.conn), _ptr(r.count),
                                  r.stream.numel(), r.cap, r.conn if one else 0)
    return arr


def launch_send_batch(sources: list[SendSource], nconns: int, closed: torch.Tensor | None, out: torch.Tensor,
                      offsets: torch.Tensor, count: torch.Tensor, conn_of: torch.Tensor, origin: torch.Tensor,
                      pos: torch.Tensor | None, queues: torch.Tensor, counts: torch.Tensor | None, status: Status,
                      ws: torch.Tensor, stream=None) -> None:
    """xdrg_rpc_send_batch as it is: closed int32 [nconns] or None, out uint8,
    offsets int64 [entries + 1] (entries = the sum of the sources' cap), count
    int64 [1], conn_of int32 [entries], origin int64 [entries], pos int64
    [entries] or None, queues int64 [4 nconns] (xdrg_rpc_wqueue records),
    counts int64 [4] or None, ws uint8 of
    xdrg_rpc_send_batch_workspace_size(entries, nconns) bytes.  `status` is not
    initialised here.  Kernels only: capturable."""
    A.check(A.lib().xdrg_rpc_send_batch(_send_srcs(sources), len(sources), nconns, _ptr(closed), _ptr(out),
                                        out.numel(), offsets.data_ptr(), count.data_ptr(), _ptr(conn_of),
                                        _ptr(origin), _ptr(pos), _ptr(queues), _ptr(counts), _ptr(ws), ws.numel(),
                                        status.ptr, _stream() if stream is None else stream),
            "xdrg_rpc_send_batch")


def wqueues_numpy(queues: torch.Tensor) -> np.ndarray:
    """Device xdrg_rpc_wqueue array -> numpy structured array (copies)."""
    return queues.cpu().numpy().view(WQUEUE_DTYPE).reshape(-1)


@dataclass
class Queued:
    """What send_batch() queued: `stream` uint8, every connection's messages
    contiguous and in putmsg order; `offsets` int64 [count + 1], the mark of
    queue position j and then the end; `count`; `conn_of` int32 [count];
    `origin` int64 [count], source << 32 | entry; `pos` int64 [entries], the
    queue position of every entry in source-major order, or SEND_DROPPED,
    SEND_EMPTY, SEND_UNUSABLE; `queues` int64 [4 nconns], the 32-byte
    xdrg_rpc_wqueue records (queues_numpy()); `counts` = (queued, dropped,
    empty, unusable)."""
    stream: torch.Tensor
    offsets: torch.Tensor
    count: int
    conn_of: torch.Tensor
    origin: torch.Tensor
    pos: torch.Tensor
    queues: torch.Tensor
    counts: tuple

    def queues_numpy(self) -> np.ndarray:
        return wqueues_numpy(self.queues)

    def ranges(self) -> np.ndarray:
        """int64 [nconns, 2]: connection c's bytes are stream[ranges[c, 0]:
        ranges[c, 1]], one writev; consecutive ranges tile the stream."""
        q = self.queues_numpy()
        b = q["begin"].astype(np.int64)
        return np.stack([b, b + q["len"].astype(np.int64)], axis=1)


def send_batch(sources: list, nconns: int, closed=None, capacity: int | None = None) -> Queued:
    """msg_sock::putmsg for many message streams and connections at once
    (xdrg_rpc_send_batch; msgsock.cc:121-134).  sources: a list of (stream,
    offsets, conn) -- see send_source() -- or SendSource, at most 64:
    ValueError beyond; putmsg order on a connection is source 0 first, each
    source in entry order.  closed: one flag per connection (a tensor, an
    array, Sender.closed()) or None; a closed connection's messages are
    dropped (wfail_, :124-127).  One sync, for the totals.  capacity: bytes of
    the output, by default the sum of the streams' bytes, which holds whatever
    sources with disjoint entries can queue; a smaller one (or overlapping
    entries) raises XdrRuntimeError (XDRG_ERR_OVERFLOW_PUT) with record = the
    first queue position that does not fit."""
    srcs = [r if isinstance(r, SendSource) else send_source(*r) for r in sources]
    if len(srcs) > A.RPC_MAX_SEND_SRCS:
        raise ValueError(f"at most {A.RPC_MAX_SEND_SRCS} message streams per call")
    dev = srcs[0].stream.device if srcs else torch.device("cuda")
    entries = sum(r.cap for r in srcs)
    cap = sum(r.stream.numel() for r in srcs) if capacity is None else capacity
    if closed is not None:
        closed = _sock_tensor(closed, nconns, dev)
    out = torch.empty(max(cap, 4), dtype=torch.uint8, device=dev)[:cap]
    offs = torch.empty(entries + 1, dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    conn_of = torch.empty(max(entries, 1), dtype=torch.int32, device=dev)[:entries]
    origin = torch.empty(max(entries, 1), dtype=torch.int64, device=dev)[:entries]
    pos = torch.empty(max(entries, 1), dtype=torch.int64, device=dev)[:entries]
    queues = torch.empty(max(4 * nconns, 4), dtype=torch.int64, device=dev)[:4 * nconns]
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    ws = torch.empty(max(A.lib().xdrg_rpc_send_batch_workspace_size(entries, nconns), 16), dtype=torch.uint8,
                     device=dev)
    e = _run_status(dev, lambda st, s: launch_send_batch(srcs, nconns, closed, out, offs, cnt, conn_of, origin, pos,
                                                         queues, counts, st, ws, s))
    n = int(cnt.item())
    return Queued(out[:int(e.total_bytes)], offs[:n + 1], n, conn_of[:n], origin[:n], pos, queues,
                  tuple(int(v) for v in counts.tolist()))


class Sender:
    """The host's wqueue_ / wstart_ / wsize_ / wfail_ (msgsock.h) for many
    connections: the messages each has queued and not yet written.  Host code
    only, the mirror of Receiver; the queueing order is send_batch's.

        tx.queue(send_batch(sources, nconns, tx.closed(nconns)))
        n = os.writev(fd, tx.iov(conn))     # msg_sock::output, msgsock.cc:157-188
        tx.wrote(conn, n)                   # or tx.fail(conn); EAGAIN: nothing
    """

    def __init__(self):
        self._queue: dict = {}   # connection -> list of memoryviews, the front one whole (wqueue_)
        self._start: dict = {}   # connection -> bytes of the front message already written (wstart_)
        self._size: dict = {}    # connection -> bytes queued and not written (wsize_)
        self.failed: set = set()  # connections with wfail_

    def putmsg(self, conn, msg) -> None:
        """msg_sock::putmsg (msgsock.cc:121-134) without the output() it
        starts: dropped after a failure, else queued whole."""
        if conn in self.failed:
            return
        m = memoryview(msg).cast("B")
        self._size[conn] = self._size.get(conn, 0) + len(m)
        self._queue.setdefault(conn, []).append(m)

    def queue(self, queued: Queued, ids=None) -> None:
        """Take every connection's range of a Queued (one download of the
        stream): putmsg for each of its messages in queue order.  ids[c] names
        connection c of the batch (default: c itself)."""
        data = queued.stream.cpu().numpy()
        offs = queued.offsets.cpu().numpy()
        for c, q in enumerate(queued.queues_numpy()):
            first, msgs = int(q["first"]), int(q["msgs"])
            conn = c if ids is None else ids[c]
            for j in range(first, first + msgs):
                self.putmsg(conn, data[int(offs[j]):int(offs[j + 1])].data)

    def pending(self, conn) -> int:
        """wsize_: bytes queued for conn and not yet written."""
        return self._size.get(conn, 0)

    def iov(self, conn, maxiov: int = 8) -> list:
        """What output() hands writev (msgsock.cc:160-172): at most maxiov
        buffers, the first from wstart_."""
        q = self._queue.get(conn, [])
        return [m[self._start.get(conn, 0):] if i == 0 else m for i, m in enumerate(q[:maxiov])]

    def wrote(self, conn, n: int) -> None:
        """pop_wbytes(n) (msgsock.cc:137-155) after a writev that returned n
        > 0 (0 is a no-op, as there)."""
        if n == 0:
            return
        if n < 0 or n > self.pending(conn):
            raise ValueError(f"wrote({conn!r}, {n}): {self.pending(conn)} bytes are queued")
        self._size[conn] -= n
        q = self._queue[conn]
        front = len(q[0]) - self._start.get(conn, 0)
        if n < front:
            self._start[conn] = self._start.get(conn, 0) + n
            return
        n -= front
        done = 1
        while n > 0 and n >= len(q[done]):
            n -= len(q[done])
            done += 1
        del q[:done]
        self._start[conn] = n

    def fail(self, conn) -> None:
        """writev failed with anything but EAGAIN (msgsock.cc:175-179): the
        queue is cleared, and whatever is queued later is dropped."""
        self.failed.add(conn)
        self._queue.pop(conn, None)
        self._start.pop(conn, None)
        self._size.pop(conn, None)

    def closed(self, nconns: int, ids=None) -> torch.Tensor:
        """The d_closed array of the next send_batch: int32 [nconns] (on the
        host), 1 where connection ids[c] (default: c) has failed."""
        t = torch.zeros(nconns, dtype=torch.int32)
        for c in range(nconns):
            if (c if ids is None else ids[c]) in self.failed:
                t[c] = 1
        return t
