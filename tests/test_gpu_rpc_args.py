"""GPU: decode_arg for a whole dispatched batch (xdrg_rpc_verify_args,
xdrg_rpc_gather_args; xdrpp/server.h:205-214, srpc.h:130-134): the calls
whose arguments do not decode become GARBAGE_ARGS one by one, the rest are
gathered per procedure and decoded with the existing kernels.

The batch is built here: 768 record-marked messages, calls of three
procedures with plans (rec128, recvar, containertest arguments), of a
registered procedure with no plan, and the non-CALL and malformed messages
of workloads.rpc_calls; every fifth call's arguments are damaged.  Expected
values: the restatement's headers (oracle_bridge.rpc_headers) with action and
err rewritten where its decode of the argument slice fails."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from xdrpp_amd import _abi as A  # noqa: E402
from xdrpp_amd import marshal as M  # noqa: E402
from xdrpp_amd import rpc as R  # noqa: E402
from xdrpp_amd import schemas as S  # noqa: E402
from xdrpp_amd import workloads as W  # noqa: E402
from xdrpp_amd.xdr_types import compile_plan  # noqa: E402
import oracle_bridge as O  # noqa: E402
import verdict_model as V  # noqa: E402

NMSG = 768
# three procedures of W.RPC_PROCS with argument plans, and one without
PROCS = {(100000, 2, 0): "rec128", (100000, 3, 1): "recvar", (100003, 3, 5): "containertest"}
NO_PLAN = (100003, 4, 7)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def be_words(words):
    return np.array(words, dtype=">u4").view(np.uint8)


class Batch:
    """The stream, its index and the numpy model of the headers after
    dispatch + verify_args."""

    def __init__(self):
        rng = np.random.default_rng(11)
        keys = list(PROCS) + [NO_PLAN]
        self.cps = {k: compile_plan(S.ALL[name]) for k, name in PROCS.items()}
        recs = {}
        for k, name in PROCS.items():  # encoded records to draw arguments from
            nat, heap = W.GENERATORS[name](NMSG)
            x, offs = O.encode(self.cps[k], nat, NMSG, heap)
            recs[k] = [x[int(offs[i]):int(offs[i + 1])] for i in range(NMSG)]
        fs, fo = W.rpc_calls(512)
        fh = O.rpc_headers(fs, fo, W.RPC_PROCS)
        foreign = [fs[int(fo[i]):int(fo[i + 1])] for i in np.nonzero(fh["action"] != A.RPC_DISPATCH)[0]]
        assert {A.RPC_DROP_MALFORMED, A.RPC_DROP_NONCALL} <= set(fh["action"].tolist())
        msgs, ncall = [], 0
        for i in range(NMSG):
            if i % 8 == 7:  # a message that is no dispatched call
                msgs.append(foreign[(i // 8) % len(foreign)])
                continue
            k = keys[int(rng.integers(len(keys)))]
            args = recs[k][i].copy() if k in recs else be_words(rng.integers(1 << 32, size=int(rng.integers(9))))
            if ncall % 5 == 0 and args.size:  # damaged: a word replaced, or words cut off / added at the end
                if (ncall // 5) % 2 == 0:
                    V.put_be(args, 4 * int(rng.integers(args.size // 4)), V.damaged_word(rng))
                else:
                    d = int(rng.integers(1, 4)) * (1 if rng.integers(2) else -1)
                    args = args[:max(args.size - 4 * -d, 0)] if d < 0 else \
                        np.concatenate([args, be_words(rng.integers(1 << 32, size=d))])
            ncall += 1
            hdr = be_words([int(rng.integers(1 << 32)), 0, 2, k[0], k[1], k[2], 0, 0, 0, 0])
            body = np.concatenate([hdr, args])
            msgs.append(np.concatenate([be_words([body.size | A.MARK_LAST]), body]))
        self.stream = np.concatenate(msgs)
        self.offsets = np.concatenate([[0], np.cumsum([m.size for m in msgs])]).astype(np.uint64)
        self.dispatched = O.rpc_headers(self.stream, self.offsets, W.RPC_PROCS)
        self.model = self.dispatched.copy()
        self.verdicts = np.zeros(NMSG, dtype=np.uint32)
        for i, h in enumerate(self.model):
            key = tuple(int(v) for v in h["w"][1:4])
            if h["action"] == A.RPC_DISPATCH and key in self.cps:
                v = V.oracle_verdict(self.cps[key], self.stream, h["body_off"], h["end"])
                self.verdicts[i] = v
                if v:
                    self.model[i]["action"] = A.RPC_GARBAGE_ARGS
                    self.model[i]["err"] = v & 0xFF

    def selected(self, key, hdrs=None):
        h = self.model if hdrs is None else hdrs
        return np.nonzero((h["action"] == A.RPC_DISPATCH) & (h["w"][:, 1] == key[0]) &
                          (h["w"][:, 2] == key[1]) & (h["w"][:, 3] == key[2]))[0]

    def slices(self, idx):
        return [self.stream[int(self.model[i]["body_off"]):int(self.model[i]["end"])] for i in idx]


@pytest.fixture(scope="module")
def batch():
    return Batch()


@pytest.fixture(scope="module")
def plans():
    return {k: M.Plan(S.ALL[name]) for k, name in PROCS.items()}


@pytest.fixture()
def on_dev(batch, dev):
    """(stream, freshly dispatched headers) on the device."""
    st = to_dev(batch.stream, dev)
    hd = R.dispatch(st, to_dev(batch.offsets.view(np.int64), dev), W.RPC_PROCS)
    assert hd.cpu().numpy().tobytes() == batch.dispatched.tobytes()
    return st, hd


def test_the_batch_is_a_test(batch):
    """Every kind of header is there, and the damage splits the calls."""
    acts = set(batch.dispatched["action"].tolist())
    assert {A.RPC_DISPATCH, A.RPC_DROP_MALFORMED, A.RPC_DROP_NONCALL} <= acts
    for key in PROCS:
        sel = batch.selected(key, batch.dispatched)
        bad = np.count_nonzero(batch.verdicts[sel])
        assert bad >= 8 and len(sel) - bad >= 64, (key, len(sel), bad)
    assert len(batch.selected(NO_PLAN)) >= 64
    assert len({int(v) & 0xFF for v in batch.verdicts if v}) >= 3  # several different errors


def test_verify_args_rewrites_only_the_failing_calls(batch, plans, on_dev):
    st, hd = on_dev
    v = R.verify_args(st, hd, plans)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), batch.verdicts)
    got = R.hdrs_numpy(hd)
    assert got.tobytes() == batch.model.tobytes()
    same = batch.verdicts == 0  # untouched headers: byte-identical to the dispatch's
    assert got[same].tobytes() == batch.dispatched[same].tobytes()
    # a second pass finds nothing left to do
    assert not R.verify_args(st, hd, plans).cpu().numpy().any()
    assert R.hdrs_numpy(hd).tobytes() == batch.model.tobytes()


def test_gather_args_per_procedure(batch, plans, on_dev):
    st, hd = on_dev
    R.verify_args(st, hd, plans)
    for key in list(PROCS) + [NO_PLAN]:
        want_idx = batch.selected(key)
        pieces = batch.slices(want_idx)
        args, offs, index = R.gather_args(st, hd, key)
        assert np.array_equal(index.cpu().numpy(), want_idx)
        want_offs = np.concatenate([[0], np.cumsum([p.size for p in pieces])])
        assert np.array_equal(offs.cpu().numpy(), want_offs)
        assert args.cpu().numpy().tobytes() == np.concatenate(pieces).tobytes()


def test_decode_args_equals_oracle(batch, plans, on_dev):
    st, hd = on_dev
    out = R.decode_args(st, hd, plans)
    assert R.hdrs_numpy(hd).tobytes() == batch.model.tobytes()
    for key, (index, native, heap) in out.items():
        want_idx = batch.selected(key)
        assert np.array_equal(index.cpu().numpy(), want_idx)
        pieces = batch.slices(want_idx)
        gathered = np.concatenate(pieces)
        offs = np.concatenate([[0], np.cumsum([p.size for p in pieces])]).astype(np.uint64)
        o_nat, o_heap = O.decode(batch.cps[key], gathered, len(pieces), offs)  # no error
        assert np.array_equal(native.cpu().numpy(), o_nat), key
        if not plans[key].is_fixed:
            assert np.array_equal(heap.cpu().numpy(), o_heap), key


def test_error_replies_of_the_rewritten_headers(batch, plans, on_dev):
    st, hd = on_dev
    R.verify_args(st, hd, plans)
    out, offs = R.error_replies(hd)
    want, want_offs, rc, _ = O.rpc_replies(batch.model)
    assert rc == 0 and out.cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(offs.cpu().numpy().view(np.uint64), want_offs)
    assert np.count_nonzero(batch.model["action"] == A.RPC_GARBAGE_ARGS) == np.count_nonzero(batch.verdicts)


def test_capacity_one_byte_short(batch, plans, on_dev):
    st, hd = on_dev
    R.verify_args(st, hd, plans)
    key = (100000, 3, 1)
    idx = batch.selected(key)
    total = sum(p.size for p in batch.slices(idx))
    args, _, _ = R.gather_args(st, hd, key, capacity=total)  # exactly enough
    assert args.numel() == total
    with pytest.raises(M.XdrRuntimeError) as ei:
        R.gather_args(st, hd, key, capacity=total - 1)
    assert ei.value.code == A.ERR_OVERFLOW_PUT and ei.value.record == idx[-1]
    # ... and half: the first message whose end passes the capacity
    ends = np.cumsum([p.size for p in batch.slices(idx)])
    with pytest.raises(M.XdrRuntimeError) as ei:
        R.gather_args(st, hd, key, capacity=total // 2)
    assert ei.value.code == A.ERR_OVERFLOW_PUT and ei.value.record == idx[np.nonzero(ends > total // 2)[0][0]]


def test_empty_batch_and_no_match(batch, plans, on_dev, dev):
    st, hd = on_dev
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    assert R.verify_args(st, empty, plans).numel() == 0
    args, offs, index = R.gather_args(st, empty, (100000, 2, 0))
    assert args.numel() == 0 and index.numel() == 0 and offs.cpu().tolist() == [0]
    assert R.decode_args(st, empty, plans)[(100000, 2, 0)][0].numel() == 0
    # no message of the batch is a call of this procedure
    args, offs, index = R.gather_args(st, hd, (100000, 2, 8))
    assert args.numel() == 0 and index.numel() == 0 and offs.cpu().tolist() == [0]
