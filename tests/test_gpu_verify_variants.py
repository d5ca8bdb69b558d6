"""Every launch variant of the verdict kernels (xdrg_verify,
xdrg_rpc_verify_args, xdrg_rpc_verify_results: k_verify, k_rpc_verify_args and
k_rpc_verify_results<SUB, LDSOPS> over verify_walk, csrc/verify_kernels.h,
replies_kernels.h) on plans either side of the LDS limit, on the fixed and var
zoos with the real reference's exceptions, and on full 64-entry plan tables.

CPU half: verify_geometry (csrc/verify_host.h) restated from the headers'
own constants, the literal table of the twelve variants with the plan or plan
table that lands in each, the op counts, and the conditions that make every
batch a test -- all on the restatement alone (verify_cases.py), so they hold
before anything runs on a GPU.

GPU half: every verdict, op index, count and header compared exactly with the
committed fixtures where they have the case and with the restatement
elsewhere.

Where the conditions of a batch cannot all hold at once they are read as
follows.  Damaged records sit at 0, 63, 64 and n - 1 *and* at every odd
record, so that the restatement calls about half of a batch bad; every other
record is intact.  A batch of one record cannot be a quarter bad: n = 1 runs
a damaged and a clean record, and the share and the codes are asserted from
n = 63 on.  STACK_GET needs a stack limit, which is per launch: it has a
batch of its own.  A plan of exactly limit + 1 ops has no failing op past the
limit (its last op is END): flat1601 and frame833 are there for that, beside
the plans of exactly 1536, 1537, 768 and 769 ops.  In the RPC batches two
calls in five are damaged, not one, so that at least a quarter is bad."""
import itertools

import numpy as np
import pytest

from xdrpp_amd import _abi as A
from xdrpp_amd import objects as OB
import oracle_bridge as O
import reply_model as RM
import verdict_model as V
import verify_cases as VC
import test_fixed_layouts as FL
import test_var_layouts as VL

gpu = pytest.mark.gpu

ENTRY_POINTS = ("xdrg_verify", "xdrg_rpc_verify_args", "xdrg_rpc_verify_results")
# what the GPU tests below are parametrised over
GPU_LIMIT_PLANS = list(VC.LIMIT_PLANS)
GPU_TABLES = list(VC.TABLES)


# ======================================================================= CPU
def test_header_constants_and_thresholds():
    """48 KiB of LDS, 128 threads and XDRG_INDEX_FRAMES (16) frames of three
    words in a workgroup with element subroutines: 1536 ops are staged
    without them, 768 with them."""
    assert VC.header_constants() == (48 << 10, 128, 16)
    assert VC.ops_limit(False) == 1536 and VC.ops_limit(True) == 768
    assert VC.geometry(False, 1536) == (False, True) and VC.geometry(False, 1537) == (False, False)
    assert VC.geometry(True, 768) == (True, True) and VC.geometry(True, 769) == (True, False)
    assert A.RPC_MAX_ARGPLANS == 64 == VC.NPLANS


def test_variant_table():
    """The twelve cells, 3 entry points x 4 variants: the restated geometry
    puts every plan and table where the literal table says."""
    assert set(VC.VARIANTS) == set(itertools.product(ENTRY_POINTS, (False, True), (False, True)))
    for (ep, sub, lds_ops), what in VC.VARIANTS.items():
        assert VC.variant_of(ep, what) == (sub, lds_ops), (ep, what)


def test_gpu_cases_cover_every_cell():
    """The cells the GPU tests run, from their parameter lists and the
    geometry: all twelve, each through the plan or table the table names."""
    ran = {("xdrg_verify",) + VC.variant_of("xdrg_verify", p): p for p in GPU_LIMIT_PLANS if p in VC.VARIANTS.values()}
    for ep in ENTRY_POINTS[1:]:
        ran.update({(ep,) + VC.variant_of(ep, t): t for t in GPU_TABLES})
    assert ran == VC.VARIANTS


@pytest.mark.parametrize("name", list(VC.LIMIT_PLANS))
def test_limit_plan_op_counts(name):
    """Exactly the stated number of ops, on the stated side of the limit; the
    hand-written records are the restatement's encode of the same values."""
    lp = VC.limit_plan(name)
    family, nops = VC.LIMIT_PLANS[name]
    assert len(lp.cp.ops) == nops == lp.nops
    assert lp.sub == (family != "flat")
    assert VC.geometry(lp.sub, nops) == (lp.sub, nops <= (768 if lp.sub else 1536))
    kinds = set(lp.cp.ops["kind"].tolist())
    if family == "flat":  # every kind the walker switches on, and both inline-vector branches
        assert {A.OP_U32, A.OP_U64, A.OP_BOOL, A.OP_ENUM, A.OP_OPAQUE, A.OP_VAROPAQUE, A.OP_STRING, A.OP_UNION,
                A.OP_JUMP, A.OP_VECTOR, A.OP_END} == kinds
        vec = [o for o in lp.cp.ops if o["kind"] == A.OP_VECTOR and not o["flags"] & A.F_POINTER]
        assert [int(o["arg2"]) for o in vec] == [1, 1, 2]  # hypers; a validated enum; that and an opaque[3]
    vals = [lp.value(r) for r in range(3)]
    nat, heap = OB.stage(lp.t, vals)
    x, _ = O.encode(lp.cp, nat, 3, heap)
    assert bytes(x) == b"".join(lp.record(r)[0] for r in range(3))


@pytest.mark.parametrize("name", list(VC.LIMIT_PLANS))
def test_limit_batches_are_tests(name):
    """On the restatement alone: a record fails exactly when it was damaged
    (a bool word of 2 is no damage), between a quarter and three quarters of
    a batch fail, the batch draws every code of the damage table, the first,
    a middle and the last op fail, and a plan past the limit fails at ops a
    staged copy could not hold."""
    lp = VC.limit_plan(name)
    one, clean = VC.limit_batch(name, 1), VC.limit_batch(name, 1, True)
    assert one.bad == 1 and clean.bad == 0
    for n in VC.NS[1:]:
        b = VC.limit_batch(name, n)
        assert [r for r in range(n) if b.want[r]] == VC.damaged_set(n) == [r for r in range(n) if b.kinds[r]]
        assert {0, 63, 64, n - 1} & set(range(n)) <= set(VC.damaged_set(n))
        assert 0.25 <= b.share <= 0.75, (n, b.share)
        assert b.codes == VC.codes_of(name), (n, sorted(b.codes))
        last = lp.nops - 2 - (VC.LITEM_OPS if lp.family == "frame" else 0)  # the record's last op before END
        assert b.ops[0] == 0 and last in b.ops
        assert any(lp.nops // 4 < op < 3 * lp.nops // 4 for op in b.ops)  # a middle op
        assert {k[:2] for k in b.kinds if k} == {d[:2] for d in lp.damages()}  # every damage is in every batch
        if name in VC.PAST:
            assert b.ops[-1] >= VC.PAST[name] and sum(op >= VC.PAST[name] for op in b.ops) >= 3, b.ops[-8:]
    if lp.family == "flat":  # both inline-vector branches fail in elements k > 0
        b = VC.limit_batch(name, 257)
        hit = {b.kinds[r][0]: int(b.want[r]) for r in range(257) if b.kinds[r]}
        vec = [i for i, o in enumerate(lp.cp.ops) if o["kind"] == A.OP_VECTOR and not o["flags"] & A.F_POINTER]
        assert hit["pv_past"] == V.verdict(vec[0] + 1, A.ERR_OVERFLOW_GET)
        assert hit["ev_enum"] == hit["ev_enum0"] == V.verdict(vec[1] + 1, A.ERR_INVALID_ENUM)
        assert hit["cv_enum"] == V.verdict(vec[2] + 1, A.ERR_INVALID_ENUM)
        assert hit["cv_pad"] == V.verdict(vec[2] + 2, A.ERR_NONZERO_PAD)

        assert any(r % 4 == 2 and not b.kinds[r] for r in range(257))  # (records with a bool word of 2)
        assert VC.limit_plan(name).bool2(2) != VC.limit_plan(name).record(2)[0]


@pytest.mark.parametrize("name", list(VC.LIMIT_PLANS))
def test_stack_batches_are_tests(name):
    """One below the depth of the deepest records: those overflow the stack,
    the shallow ones decode."""
    b = VC.stack_batch(name)
    assert b.codes == {A.ERR_STACK_GET} and 0.25 <= b.share <= 0.75, b.share
    assert not V.oracle_verdicts(VC.limit_plan(name).cp, b.x, b.spans[:8]).any()  # (the limit alone fails them)


@pytest.mark.parametrize("table", list(VC.TABLES))
def test_tables_are_full_and_land_in_their_variant(table):
    names = VC.TABLES[table]
    assert len(names) == A.RPC_MAX_ARGPLANS
    es = [VC.entry(n) for n in names]
    sub, over = "sub" in table, "over" in table
    assert any(e.sub for e in es) == sub
    total = sum(e.nops for e in es)
    assert (total <= VC.ops_limit(sub)) == (not over), total
    assert VC.table_geometry(names) == (sub, not over)
    assert VC.table_geometry(names, VC.VOID_SLOTS) == (sub, not over)  # as result plans, voids left out
    keys = [VC.slot_key(k) for k in range(VC.NPLANS)]
    assert keys == sorted(keys) and len({k[0] for k in keys}) == 2
    if over:
        assert names[VC.SWAP_SLOT] in VC.PAST and [a for a, b in zip(names, VC.TABLES[table[:-5]]) if a != b] == \
            [names[VC.SWAP_SLOT]]


@pytest.mark.parametrize("table", list(VC.TABLES))
def test_arg_batches_are_tests(table):
    """On the restatement alone: every kind of header, between a quarter and
    three quarters of the dispatched calls with a plan bad, every damaged
    call among them, good and damaged calls for the first, the last and the
    swapped table slot, every slot called."""
    b = VC.arg_batch(table)
    acts = set(b.dispatched["action"].tolist())
    assert {A.RPC_DISPATCH, A.RPC_DROP_MALFORMED, A.RPC_DROP_NONCALL} <= acts
    bad = np.count_nonzero(b.verdicts[b.planned])
    assert 0.25 <= bad / len(b.planned) <= 0.75
    assert sorted(np.nonzero(b.verdicts)[0]) == b.damaged_calls
    for k in (0, VC.NPLANS - 1, VC.SWAP_SLOT):
        sel = b.selected(b.keys[k], b.dispatched)
        nbad = np.count_nonzero(b.verdicts[sel])
        assert nbad >= 1 and len(sel) - nbad >= 1, (k, len(sel), nbad)
    assert all(len(b.selected(key, b.dispatched)) >= 3 for key in b.keys)
    assert len(b.selected(VC.NO_PLAN, b.dispatched)) >= 3 and len(b.selected(VC.UNREG, b.dispatched)) == 0
    assert len({int(v) & 0xFF for v in b.verdicts if v}) >= 6
    # a wave's lanes hold (nearly) as many plans as it has calls
    wave = [tuple(int(v) for v in h["w"][1:4]) for h in b.dispatched[:64] if h["action"] == A.RPC_DISPATCH]
    assert len(set(wave)) == len(wave) >= 56


@pytest.mark.parametrize("table", list(VC.TABLES))
def test_result_batches_are_tests(table):
    b = VC.result_batch(table)
    acts = set(b.matched["action"].tolist())
    assert {A.RPCR_OK, A.RPCR_ACCEPT_STAT, A.RPCR_AUTH_STAT, A.RPCR_RPCVERS_MISMATCH, A.RPCR_NOT_REPLY,
            A.RPCR_MALFORMED, A.RPCR_UNKNOWN_XID} <= acts
    bad = np.count_nonzero(b.verdicts[b.planned])
    assert 0.25 <= bad / len(b.planned) <= 0.75
    assert VC.RES_BASE > 0 and 0 in VC.VOID_SLOTS and VC.NPLANS - 1 not in VC.VOID_SLOTS
    res = b.res[np.clip(b.call, 0, None)]
    for k in (0, 1, VC.VOID_SLOTS[1], VC.SWAP_SLOT, VC.NPLANS - 1):  # a void and a real slot at either end
        sel = [i for i in b.planned if res[i] == VC.RES_BASE + k]
        nbad = np.count_nonzero(b.verdicts[sel])
        assert nbad >= 1 and len(sel) - nbad >= 1, (k, len(sel), nbad)
    void = [i for i in b.planned if b.cps[int(res[i])] is None]
    assert {int(b.matched["end"][i] - b.matched["body_off"][i]) for i in void} == {0, 4}  # trailing bytes
    assert {int(b.verdicts[i]) for i in void} == {0, V.verdict(V.RECORD_LEVEL, A.ERR_TRAILING)}
    # ... and 2: no whole words, so the header check calls the message malformed before the result is looked at
    last = VC.NMSG - 1
    assert b.call[last] >= 0 and b.cps[int(res[last])] is None and b.matched["action"][last] == A.RPCR_MALFORMED
    assert int(b.offsets[last + 1] - b.offsets[last]) == 4 + 24 + 2
    assert b.verdicts[last] == V.verdict(V.RECORD_LEVEL, A.ERR_SIZE_NOT_MULT4)
    assert b.model["action"][last] == A.RPCR_GARBAGE_RES
    f, fv = VC.forged_void(b)  # a void reply's header forged to 2 result bytes reaches the void walk's own test
    assert list(fv).count(V.verdict(V.RECORD_LEVEL, A.ERR_SIZE_NOT_MULT4)) == 1
    assert np.count_nonzero(b.reply_of < 0) >= 32  # calls never answered
    assert any(int(r) in VC.NO_PLAN_RES for r in res[b.call >= 0])


# ======================================================================= GPU
def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_plans = {}


def plan_of(name, cp):
    """One device plan per layout; verify uses no generated kernel."""
    from xdrpp_amd import marshal as M
    if name not in _plans:
        _plans[name] = M.Plan(cp, {"specialize": 0})
    return _plans[name]


def marshaler(name, cp, dev):
    from xdrpp_amd import marshal as M
    return M.Marshaler(plan_of(name, cp), dev)


def run_spans(mar, dx, spans, stack_limit=A.DEFAULT_STACK_LIMIT, stride16=False):
    """(uint32 verdicts, bad_count) over begin / end arrays, each contiguous
    (an 8-byte stride), or interleaved in one array (a 16-byte stride)."""
    spans = np.ascontiguousarray(spans, dtype=np.int64)
    if stride16:
        be = _dev(spans, mar.device)
        b, e = be[:, 0], be[:, 1]
    else:
        b, e = _dev(spans[:, 0].copy(), mar.device), _dev(spans[:, 1].copy(), mar.device)
    v, bad = mar.verify(dx, begin=b, end=e, stack_limit=stack_limit)
    return v.cpu().numpy().view(np.uint32), bad


def check_batch(mar, b, stride16=False):
    got, bad = run_spans(mar, _dev(b.x, mar.device), b.spans, b.stack_limit, stride16)
    wrong = np.nonzero(got != b.want)[0]
    assert wrong.size == 0, (b.n, [(int(r), b.kinds[r], hex(got[r]), hex(b.want[r])) for r in wrong[:6]])
    assert bad == b.bad


@gpu
@pytest.mark.parametrize("name", GPU_LIMIT_PLANS)
def test_limit_plans_gpu(dev, name):
    """A plan at, one past and well past the LDS limit, with and without
    element subroutines and frames: batches of 1, 63, 64, 65 and 257 records,
    half of them damaged where the answer is known, through contiguous and
    (n = 65) interleaved begin / end arrays and through an offsets array;
    then intact records under a stack limit one below their depth.  Every
    verdict, its op index and bad_count are the restatement's."""
    lp = VC.limit_plan(name)
    mar = marshaler(name, lp.cp, dev)
    check_batch(mar, VC.limit_batch(name, 1, True))
    for n in VC.NS:
        check_batch(mar, VC.limit_batch(name, n))
    check_batch(mar, VC.limit_batch(name, 65), stride16=True)
    check_batch(mar, VC.stack_batch(name))
    b = VC.stack_batch(name)  # the same records at the default limit, by their offsets: all decode
    v, bad = mar.verify(_dev(b.x[:int(b.offsets[-1])], dev), _dev(b.offsets, dev))
    assert not v.cpu().numpy().any() and bad == 0


def check_reference_case(plan, mar, d, x, offs, spans, want, exc, dev, implied=False, decode=True):
    """One damage case of a fixture in the records EDGES of 257: each of them
    gets the reference's exception and what() and the restatement's op, every
    other record 0, bad_count 4; the decode of the same batch fails at record
    0 with verdicts[0]'s code and op."""
    from xdrpp_amd import marshal as M
    dx = _dev(x, dev)
    runs = [run_spans(mar, dx, spans)]
    if implied:
        v, bad = mar.verify(dx[:int(offs[-1])])
        runs.append((v.cpu().numpy().view(np.uint32), bad))
    for got, bad in runs:
        assert np.array_equal(got, want), (d["kind"], np.nonzero(got != want)[0][:6])
        assert bad == 4 and list(np.nonzero(got)[0]) == list(VC.EDGES)
    for r in VC.EDGES:
        code, op = int(want[r]) & 0xFF, int(want[r]) >> 8
        assert code == A.ERR_BAD_DISCRIMINANT if d["kind"] == "discriminant" else code in VC.codes_of_what(d["what"])
        e = M.verdict_error(plan, int(want[r]), r)
        assert type(e) is exc[d["exception"]] and str(e) == d["what"] and e.record == r
        assert e.op == (None if op == V.RECORD_LEVEL else op)
    if decode:
        with pytest.raises(M.XdrRuntimeError) as ei:
            mar.decode(dx[:int(offs[-1])], VC.ZOO_N, None if implied else _dev(offs, dev))
        e = ei.value
        assert (e.record, e.code, e.op) == (0, int(want[0]) & 0xFF, int(want[0]) >> 8), (d["kind"], e.record, e.code, e.op)


@gpu
@pytest.mark.parametrize("name", list(FL.ZOO))
def test_fixed_zoo_gpu(dev, name):
    """The 17 fixed layouts at 257 records (the fixture's 8, then the
    module's), through implied offsets and explicit spans: clean, every
    damage case of the fixture, and for the layouts without one moved span
    ends and bool words of 2."""
    zb = VC.fixed_zoo(name)
    plan = plan_of(name, zb.cp)
    mar = marshaler(name, zb.cp, dev)
    dx = _dev(zb.x, dev)
    got, bad = run_spans(mar, dx, zb.spans)
    assert not got.any() and bad == 0
    v, bad = mar.verify(dx[:int(zb.offsets[-1])])
    assert v.numel() == VC.ZOO_N and not v.cpu().numpy().any() and bad == 0
    ds = VC._fixed_gold()[name]["damaged"]
    assert (not ds) == (name in VC.FIXED_UNDAMAGED)
    for k in range(len(ds)):
        d, (x, offs, spans, want) = VC.fixed_damaged(name, k)
        check_reference_case(plan, mar, d, x, offs, spans, want, FL.EXC, dev, implied=True)
    if not ds:
        x, offs, spans, want = zb.case({}, VC.MOVES)
        assert [int(w) & 0xFF for w in want[list(VC.EDGES)]] == [A.ERR_OVERFLOW_GET, A.ERR_TRAILING,
                                                                  A.ERR_SIZE_NOT_MULT4, A.ERR_OVERFLOW_GET]
        got, bad = run_spans(mar, _dev(x, dev), spans)
        assert np.array_equal(got, want) and bad == 4
    if name in VC.FIXED_BOOLS:
        x, offs, spans, want = VC.fixed_bool2(name)
        assert not want.any() and not np.array_equal(x, zb.x)
        got, bad = run_spans(mar, _dev(x, dev), spans)
        assert not got.any() and bad == 0
    else:
        assert A.OP_BOOL not in zb.cp.ops["kind"] or ds


@gpu
@pytest.mark.parametrize("name", VL.NAMES)
def test_var_zoo_gpu(dev, name):
    """The 15 var layouts at 257 records (the fixture's 16 twice, then the
    module's): clean, and every damage case of the fixture in records 0, 63,
    64 and 256 at once, each of which is the fixture's own record of that
    case."""
    zb = VC.var_zoo(name)
    plan = plan_of(name, zb.cp)
    mar = marshaler(name, zb.cp, dev)
    v, bad = mar.verify(_dev(zb.x[:int(zb.offsets[-1])], dev), _dev(zb.offsets, dev))
    assert v.numel() == VC.ZOO_N and not v.cpu().numpy().any() and bad == 0
    ds = VL._gold()[name]["damaged"]
    assert ds
    for k in range(len(ds)):
        d, (x, offs, spans, want) = VC.var_damaged(name, k)
        check_reference_case(plan, mar, d, x, offs, spans, want, VL.EXC, dev, decode=not d["resize"])


@gpu
@pytest.mark.parametrize("seed", FL.GEN_SEEDS)
def test_generated_fixed_schemas_gpu(dev, seed):
    """The 40 generated fixed schemas at 257 records, every third span end
    moved, against the restatement."""
    cp, x, spans, want = VC.gen_case(seed)
    assert np.count_nonzero(want) == len(range(1, VC.ZOO_N, 3))
    mar = marshaler(f"gen{seed}", cp, dev)
    got, bad = run_spans(mar, _dev(x, dev), spans)
    assert np.array_equal(got, want) and bad == np.count_nonzero(want)


def table_plans(names, keys):
    return {key: plan_of(n, VC.entry(n).cp) for key, n in zip(keys, names)}


@gpu
@pytest.mark.parametrize("table", GPU_TABLES)
def test_rpc_args_full_table_gpu(dev, table):
    """xdrg_rpc_verify_args over a table of 64 plans (all four variants):
    exact verdicts, headers byte-identical to the model (GARBAGE_ARGS and err
    for the failing calls, every other header untouched), a second pass that
    finds nothing, and gather_args + decode of the first and last procedure
    equal to the restatement."""
    from xdrpp_amd import marshal as M
    from xdrpp_amd import rpc as R
    b = VC.arg_batch(table)
    plans = table_plans(b.names, b.keys)
    st = _dev(b.stream, dev)
    hd = R.dispatch(st, _dev(b.offsets.view(np.int64), dev), b.procs)
    assert hd.cpu().numpy().tobytes() == b.dispatched.tobytes()
    v = R.verify_args(st, hd, plans).cpu().numpy().view(np.uint32)
    wrong = np.nonzero(v != b.verdicts)[0]
    assert wrong.size == 0, [(int(i), hex(v[i]), hex(b.verdicts[i])) for i in wrong[:6]]
    got = R.hdrs_numpy(hd)
    assert got.tobytes() == b.model.tobytes()
    same = b.verdicts == 0
    assert got[same].tobytes() == b.dispatched[same].tobytes()
    assert not R.verify_args(st, hd, plans).cpu().numpy().any()
    assert R.hdrs_numpy(hd).tobytes() == b.model.tobytes()
    for key in (b.keys[0], b.keys[-1]):
        idx = b.selected(key)
        pieces = b.slices(idx)
        args, offs, index = R.gather_args(st, hd, key)
        assert np.array_equal(index.cpu().numpy(), idx) and len(idx) >= 1
        data, want_offs = RM.gathered(pieces)
        assert np.array_equal(offs.cpu().numpy().view(np.uint64), want_offs)
        assert args.cpu().numpy().tobytes() == data.tobytes()
        native, heap = M.Marshaler(plans[key], dev).decode(args, len(idx), offs)
        o_nat, o_heap = O.decode(b.cps[key], data, len(idx), want_offs)
        assert np.array_equal(native.cpu().numpy(), o_nat), key
        if not plans[key].is_fixed:
            assert np.array_equal(heap.cpu().numpy(), o_heap), key


@gpu
@pytest.mark.parametrize("table", GPU_TABLES)
def test_rpc_results_full_table_gpu(dev, table):
    """xdrg_rpc_verify_results over the same tables as result types
    RES_BASE .. RES_BASE + 63 (one launch, a non-zero res_base, void entries
    between the real ones from slot 0 on): exact verdicts and headers, a
    second pass that finds nothing, and gather_results + decode of the first
    real and the last slot equal to the restatement."""
    from xdrpp_amd import marshal as M
    from xdrpp_amd import rpc as R
    b = VC.result_batch(table)
    plans = {r: None if e is None else plan_of(e.name, e.cp) for r, e in b.entries.items()}
    assert R._res_runs(plans) == [list(range(VC.RES_BASE, VC.RES_BASE + VC.NPLANS))]
    st, od = _dev(b.stream, dev), _dev(b.offsets.view(np.int64), dev)
    pending = R.PendingCalls(b.xids, b.res, dev)
    hd, call, reply_of = R.match_replies(st, od, pending)
    assert np.array_equal(call.cpu().numpy(), b.call) and np.array_equal(reply_of.cpu().numpy(), b.reply_of)
    assert R.hdrs_numpy(hd).tobytes() == b.matched.tobytes()
    v = R.verify_results(st, hd, call, pending, plans).cpu().numpy().view(np.uint32)
    wrong = np.nonzero(v != b.verdicts)[0]
    assert wrong.size == 0, [(int(i), hex(v[i]), hex(b.verdicts[i])) for i in wrong[:6]]
    got = R.hdrs_numpy(hd)
    assert got.tobytes() == b.model.tobytes()
    same = b.verdicts == 0
    assert got[same].tobytes() == b.matched[same].tobytes()
    assert not R.verify_results(st, hd, call, pending, plans).cpu().numpy().any()
    assert R.hdrs_numpy(hd).tobytes() == b.model.tobytes()
    for r in (VC.RES_BASE + 1, VC.RES_BASE + VC.NPLANS - 1):
        idx = RM.selected(b.stream, b.model, b.call, b.res, r)
        data, want_offs = RM.gathered(RM.slices(b.stream, b.model, idx))
        out, offs, index = R.gather_results(st, hd, call, pending, r)
        assert np.array_equal(index.cpu().numpy(), idx) and len(idx) >= 1
        assert np.array_equal(offs.cpu().numpy().view(np.uint64), want_offs)
        assert out.cpu().numpy().tobytes() == data.tobytes()
        native, heap = M.Marshaler(plans[r], dev).decode(out, len(idx), offs)
        o_nat, o_heap = O.decode(b.cps[r], data, len(idx), want_offs)
        assert np.array_equal(native.cpu().numpy(), o_nat), r
        if not plans[r].is_fixed:
            assert np.array_equal(heap.cpu().numpy(), o_heap), r
    # one void reply's header forged to hold 2 result bytes, the void results alone
    forged, want = VC.forged_void(b)
    hd = _dev(forged.view(np.uint8).reshape(-1), dev)
    voids = {VC.RES_BASE + k: None for k in VC.VOID_SLOTS[:1]}
    v = R.verify_results(st, hd, call, pending, voids).cpu().numpy().view(np.uint32)
    assert np.array_equal(v, want)
