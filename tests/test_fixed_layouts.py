"""The fixed-layout kernels (k_fixed_reg, _tile, _grp, _lds; csrc/kernels.h,
run_fixed in csrc/xdrgpu.hip) on awkward layouts.

CPU part: the layouts of oracle/x/fixedzoo.x, described here with the
xdr_types descriptors, are held to bytes the REAL reference produced over
genuine xdrc output (tests/golden/fixed.json, `make -C oracle fixed`):
sizeof/offsetof, xdr_to_opaque, xdr_from_opaque and its what() on damaged
streams.  That pins the C restatement (oracle_bridge) on these layouts; the
generated schemas further down rest on it.

GPU part: every case is bit-exact against the fixture where it has the case
and the restatement otherwise, and every case asserts which kernel it ran:
`kernels()` restates run_fixed's dispatch over xdrg_plan_fixed_shape and
xdrg_plan_get_info, so a layout that falls to another kernel fails its test
instead of passing on the wrong path.
"""
import ctypes as C
import hashlib
import json
import math
import os
import time

import numpy as np
import pytest

from conftest import GOLD, ROOT

from xdrpp_amd import _abi as A
from xdrpp_amd import marshal as M
from xdrpp_amd import schemas as S
from xdrpp_amd.xdr_types import (Bool, Double, Enum, Float, Hyper, Int, OpaqueArray, Struct, UHyper,
                                 UInt, XArray, compile_plan)
import oracle_bridge as O

gpu = pytest.mark.gpu
REF = "/root/reference"

# ------------------------------------------------------- oracle/x/fixedzoo.x
ztag = Enum("ztag", {"ZNEG": -7, "ZONE": 1, "ZBIG": 1000}, validate=True)
vpair = Struct("vpair", [("h", Hyper), ("b", Bool)])
ZOO = {t.name: t for t in [
    Struct("id16_bool", [("a", Bool), ("i", Int), ("b", Bool), ("j", Int)]),
    Struct("id32_mix", [("b", Bool), ("i", Int), ("o", OpaqueArray(7)), ("j", Int), ("e", ztag),
                        ("h", Hyper)]),
    Struct("id48_pad", [("o", OpaqueArray(5)), ("i", Int), ("j", Int), ("h", Hyper), ("u", UHyper),
                        ("k", Int), ("f", Float), ("d", Double)]),
    Struct("id80_enum", [("o", OpaqueArray(6)), ("e", ztag), ("i", Int), ("h1", Hyper), ("h2", UHyper),
                         ("d", Double), ("a", Int), ("b", UInt), ("h3", Hyper), ("f", Float),
                         ("e2", ztag), ("h4", Hyper), ("t0", Int), ("t1", Int)]),
    Struct("id112", [("a", Int), ("b", Int), ("h", XArray(Hyper, 5)), ("c", XArray(Int, 2)),
                     ("g", XArray(Hyper, 7))]),
    Struct("id208", [("h", XArray(Hyper, 11)), ("i", XArray(Int, 6)), ("g", XArray(Hyper, 12))]),
    Struct("lastbool", [("h", Hyper), ("i", Int), ("b", Bool)]),
    Struct("bool4", [("a", Bool), ("b", Bool), ("c", Bool), ("d", Bool), ("i", Int)]),
    Struct("bytes124", [("a", OpaqueArray(1)), ("b", OpaqueArray(2)), ("c", OpaqueArray(1)), ("i", Int)]),
    Struct("tailbools", [("i", Int), ("a", Bool), ("b", Bool)]),
    Struct("enumpad", [("e", ztag), ("o", OpaqueArray(3)), ("b", Bool), ("f", ztag)]),
    Struct("wide16", [("a", Bool), ("b", Bool), ("i", Int), ("h", Hyper), ("j", Int), ("g", Hyper),
                      ("k", XArray(Int, 8))]),
    Struct("odd7", [("a", Bool), ("b", Bool), ("i", XArray(Int, 6))]),
    vpair,
    Struct("arr5", [("v", XArray(vpair, 5)), ("t", Bool)]),
    Struct("big10k", [("o", OpaqueArray(10001)), ("i", Int), ("b", Bool)]),
    Struct("big20k", [("o", OpaqueArray(20001)), ("i", Int)]),
]}
BIG = ("big10k", "big20k")
# not in the fixture (the restatement is their oracle): the smallest record
# whose 4-record LDS tiles number more than the kernel's 4096 workgroups at a
# batch of 16,388, and a record no LDS tile can hold
big8k = Struct("big8k", [("o", OpaqueArray(8193)), ("i", Int)])
big50k = Struct("big50k", [("o", OpaqueArray(50001)), ("i", Int)])
# records whose 4-record tile and program pass 160 KiB of LDS (224 and 252 KB)
# and that fit with 2 records and with 1 record per tile (9,001 words: no
# 16-byte tile rows, so the aligned launch is word by word as well)
big32k = Struct("big32k", [("o", OpaqueArray(32001)), ("i", Int)])
big36k = Struct("big36k", [("o", OpaqueArray(35997)), ("i", Int)])
IDENTITY = {"id16_bool": 1, "id32_mix": 2, "id48_pad": 3, "id80_enum": 5, "id112": 7, "rec128": 8,
            "id208": 13, "lastbool": 1}  # chunks per record


def struct_of(name):
    return S.ALL[name] if name in ("rec128", "numerics") else ZOO[name]


@pytest.fixture(scope="module")
def zoo_gold():
    with open(os.path.join(GOLD, "fixed.json")) as f:
        return json.load(f)["structs"]


_cps = {}


def cp_of(name):
    if name not in _cps:
        _cps[name] = compile_plan(struct_of(name))
    return _cps[name]


def fields_of(cp):
    """(op index, kind, flags, native offset, wire offset, arg0, arg1) of a fixed plan's fields."""
    out, w = [], 0
    for i, o in enumerate(cp.ops):
        k = int(o["kind"])
        if k == A.OP_END:
            break
        out.append((i, k, int(o["flags"]), int(o["noff"]), w, int(o["arg0"]), int(o["arg1"])))
        w += 8 if k == A.OP_U64 else ((int(o["arg0"]) + 3) & ~3) if k == A.OP_OPAQUE else 4
    assert w == cp.fixed_size
    return out


def big_native(name, g):
    """The big structs' records from the fixture's field values."""
    t = ZOO[name]
    nat = np.zeros((len(g["values"]), t.size), dtype=np.uint8)
    for r, v in enumerate(g["values"]):
        n = dict(t.fields)["o"].n
        start, step = v["o"]
        nat[r, :n] = (start + np.arange(n, dtype=np.uint64) * step).astype(np.uint8)
        nat[r, t.offsets["i"]:t.offsets["i"] + 4] = np.frombuffer(np.int32(v["i"]).tobytes(), dtype=np.uint8)
        if "b" in v:
            nat[r, t.offsets["b"]] = v["b"]
    return nat.reshape(-1)


def unhex(s):
    return np.frombuffer(bytes.fromhex(s), dtype=np.uint8).copy()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def gold_native(name, g):
    if name in BIG:
        nat = big_native(name, g)
        assert sha(nat) == g["native_sha256"]
        return nat
    return unhex(g["native"])


# ======================================================================= CPU
@pytest.mark.parametrize("name", list(ZOO))
def test_layout_equals_cxx(zoo_gold, name):
    """The staged native layout is the C++ layout xdrc generates."""
    t, g = ZOO[name], zoo_gold[name]
    assert (t.size, t.align, t.fixed_wire) == (g["sizeof"], g["alignof"], g["wire"])
    assert t.offsets == g["offsetof"]
    cp = cp_of(name)
    assert (cp.stride, cp.fixed_size) == (g["sizeof"], g["wire"])


@pytest.mark.parametrize("name", list(ZOO))
def test_descriptors_equal_fixedzoo_x(name):
    """The descriptors above are the types of oracle/x/fixedzoo.x (every
    enum of its namespace validated, as ref_fixed.cc declares)."""
    import xdrc_front as xdrc
    from test_xdrc import same_plan
    sp = xdrc.load_file(os.path.join(ROOT, "oracle", "x", "fixedzoo.x"), validate_enums=("ztag",))
    assert same_plan(sp.plan(name), cp_of(name))


@pytest.mark.skipif(not os.path.exists(f"{REF}/xdrpp/marshal.cc"), reason="reference tree absent")
def test_fixture_regenerates(tmp_path):
    """fixed.json is what the reference produces today (empty diff)."""
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/ref_fixed"], check=True)
    out = tmp_path / "f.json"
    subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_fixed"), str(out)], check=True)
    assert out.read_bytes() == open(os.path.join(GOLD, "fixed.json"), "rb").read()


@pytest.mark.parametrize("name", list(ZOO))
def test_restatement_encode_equals_reference(zoo_gold, name):
    g = zoo_gold[name]
    nat = gold_native(name, g)
    x, _ = O.encode(cp_of(name), nat, 8)
    if name in BIG:
        assert sha(x) == g["xdr_sha256"] and bytes(x[:64]).hex() == g["xdr_head"]
    else:
        assert bytes(x).hex() == g["xdr"]


@pytest.mark.parametrize("name", list(ZOO))
def test_restatement_decode_equals_reference(zoo_gold, name):
    g = zoo_gold[name]
    if name in BIG:  # (the stream: test_restatement_encode_equals_reference)
        x, _ = O.encode(cp_of(name), gold_native(name, g), 8)
        nat, _ = O.decode(cp_of(name), x, 8)
        assert sha(nat) == g["decoded_sha256"]
    else:
        nat, _ = O.decode(cp_of(name), unhex(g["xdr"]), 8)
        assert bytes(nat).hex() == g["decoded"]


def gold_wire(name, g):
    return O.encode(cp_of(name), gold_native(name, g), 8)[0] if name in BIG else unhex(g["xdr"])


def damaged_cases():
    with open(os.path.join(GOLD, "fixed.json")) as f:
        z = json.load(f)["structs"]
    return [(n, k) for n in z for k in range(len(z[n]["damaged"]))]


EXC = {"xdr_should_be_zero": M.XdrShouldBeZero, "xdr_invariant_failed": M.XdrInvariantFailed}


def damage(x, W, d):
    p = d["at_record"] * W + d["offset"]
    if d["kind"] == "enum":
        x[p:p + 4] = (0, 0, 0, d["value"])
    else:
        x[p] = d["value"]


def op_at(cp, wire_off):
    """The op whose wire bytes hold wire_off."""
    return [f[0] for f in fields_of(cp) if f[4] <= wire_off][-1]


@pytest.mark.parametrize("name,k", damaged_cases())
def test_restatement_damaged_equals_reference(zoo_gold, name, k):
    """The reference's exception class, what() and first failing record."""
    g = zoo_gold[name]
    d = g["damaged"][k]
    cp = cp_of(name)
    x = gold_wire(name, g)
    damage(x, g["wire"], d)
    with pytest.raises(O.OracleError) as ei:
        O.decode(cp, x, 8)
    e = ei.value
    assert e.record == d["record"] == d["at_record"] and e.op == op_at(cp, d["offset"])
    err = M.error_from(M.Plan(cp), A.XdrgError(code=e.code, record=e.record, op=e.op))
    assert type(err) is EXC[d["exception"]] and str(err) == d["what"]
    assert A.lib().xdrg_error_message(e.code).decode() == d["what"]


# ------------------------------------------------------ which kernel runs
MALL = 256 << 20  # kMallBytes


def shape(plan, decode):
    s = A.XdrgFixedShape()
    A.check(A.lib().xdrg_plan_fixed_shape(plan.handle, int(decode), C.byref(s)), "xdrg_plan_fixed_shape")
    return s


def reg_grid(cpr, n, fs=-1):
    """k_fixed_reg's launch: (non-temporal, workgroups, grid-stride trips)."""
    nchunks = n * cpr
    ws = nchunks * 32
    nt = ws > MALL if fs < 0 else fs in (1, 3)
    one_shot = ws > 4 * MALL if fs < 0 else fs in (1, 2)
    blocks = (nchunks + 255) // 256
    if not one_shot:
        blocks = min(blocks, 1024)
    g0 = cpr // math.gcd(cpr, 256)
    blocks = (max(blocks, 1) + g0 - 1) // g0 * g0
    return nt, blocks, (nchunks + blocks * 256 - 1) // (blocks * 256)


def kernels(plan, decode, n, opts=None, aligned=True):
    """run_fixed's dispatch (csrc/xdrgpu.hip), restated: the kernels one
    encode or decode of n records launches, with their template arguments."""
    opts = opts or {}
    sh = shape(plan, decode)
    checks = bool(sh.has_checks)
    fp = opts.get("fixed_path", 0)
    if plan.path == A.PATH_FIXED_REG and aligned:
        nt, _, _ = reg_grid(plan.fixed_size // 16, n, opts.get("fixed_stream", -1))
        return [("reg", bool(sh.has_bool), checks, nt)]
    if (not checks and fp == 0 and aligned and 0 < sh.in_words <= 16 and 0 < sh.out_words <= 16
            and sh.max_terms in (1, 2)):
        return [("tile", sh.max_terms)]
    out = []
    if sh.grp_G and not checks and fp != 2 and aligned and n >= sh.grp_G:
        kt = sh.grp_KT
        u = opts.get("grp_unroll", 0) or {1: 4, 2: 2, 4: 1}[kt]
        u = {1: u if u in (1, 2) else 4, 2: 1 if u == 1 else 2, 4: 1}[kt]
        out.append(("grp", kt, u, bool(opts.get("grp_nontemporal", 0))))
        n %= sh.grp_G
        if n == 0:
            return out
    out.append(("lds", checks, aligned))  # (VEC: also 4 | records per tile, true unless the LDS limit shrank it)
    return out


def test_shape_query():
    """xdrg_plan_fixed_shape on known programs; a var plan has none."""
    p = M.Plan(ZOO["bool4"])
    e, d = shape(p, 0), shape(p, 1)
    assert (e.in_words, e.out_words, e.max_terms, e.has_bool, e.has_checks) == (2, 5, 1, 1, 0)
    assert (d.in_words, d.out_words, d.max_terms, d.has_bool, d.has_checks) == (5, 2, 4, 1, 0)
    assert (e.grp_G, e.grp_C, e.grp_KT) == (4, 5, 1) and (d.grp_G, d.grp_C, d.grp_KT) == (4, 2, 4)
    p = M.Plan(ZOO["enumpad"])
    assert (shape(p, 0).has_checks, shape(p, 1).has_checks) == (0, 1)
    p = M.Plan(ZOO["bytes124"])
    assert (shape(p, 1).grp_G, shape(p, 1).grp_KT, shape(p, 1).max_terms) == (2, 2, 2)
    s = A.XdrgFixedShape()
    assert A.lib().xdrg_plan_fixed_shape(M.Plan(S.recvar).handle, 0, C.byref(s)) == -3
    assert A.lib().xdrg_plan_fixed_shape(None, 0, C.byref(s)) == -1


def test_zoo_paths():
    """The identity layouts are the register path's, with the chunk counts
    the register-kernel cases name; everything else is not."""
    for name in list(ZOO) + ["rec128", "numerics"]:
        p = M.Plan(struct_of(name))
        if name in IDENTITY:
            assert p.path == A.PATH_FIXED_REG and p.fixed_size == 16 * IDENTITY[name], name
        else:
            assert p.path == A.PATH_FIXED_LDS, name


def test_word_index_limit():
    """Word indices are 16 bits: a record of more than 65535 words is refused
    by xdrg_plan_create, one of exactly 65535 is a plan."""
    for nbytes, want in ((4 * 65535 - 4, A.OK), (4 * 65535, -3)):
        cp = compile_plan(Struct("huge", [("o", OpaqueArray(nbytes)), ("i", Int)]))
        h = C.c_void_p()
        rc = A.lib().xdrg_plan_create(cp.ops.ctypes.data_as(C.POINTER(A.XdrgOp)), len(cp.ops), None, 0,
                                      cp.stride, C.byref(h))
        assert rc == want
        if rc == A.OK:
            A.lib().xdrg_plan_destroy(h)


# -------------------------------------------------------- generated schemas
plain_tag = Enum("ptag", {"A": 0, "B": 5, "C": -2})
SCALARS = [Int, UInt, Hyper, UHyper, Float, Double, ztag, plain_tag]


def gen_schema(seed):
    """3-24 fields of int, unsigned, hyper, float, double, bool, plain or
    validated enum, opaque[0..9], nested structs of those and T x[1..4];
    always a 4-byte scalar, so the stride is a multiple of 4.  The seed
    also picks a flavour: any field kind, word scalars only (layouts that
    can be identity), or mostly bools and short opaques (many terms per
    word)."""
    rng = np.random.default_rng(seed)
    flavour = int(rng.integers(0, 4))  # 0, 1: any; 2: scalars; 3: bytes

    def leaf():
        if flavour == 2:
            return SCALARS[int(rng.integers(0, len(SCALARS)))]
        k = int(rng.integers(0, 10 if flavour != 3 else 4))
        if k < 3 and flavour == 3:
            return Bool
        if k in (3, 8):
            return OpaqueArray(int(rng.integers(0, 10)))
        if k == 9:
            return Bool
        return SCALARS[int(rng.integers(0, len(SCALARS)))]

    def field(depth):
        r = int(rng.integers(0, 10))
        if r == 0 and depth < 2 and flavour != 2:
            t = Struct(f"s{seed}_{int(rng.integers(1 << 30))}",
                       [(f"m{i}", field(depth + 1)) for i in range(int(rng.integers(1, 4)))])
        else:
            t = leaf()
        if int(rng.integers(0, 5)) == 0 and not isinstance(t, OpaqueArray):
            t = XArray(t, int(rng.integers(1, 5)))
        return t

    fields = [(f"f{i}", field(0)) for i in range(int(rng.integers(2, 24)))]
    fields.insert(int(rng.integers(0, len(fields) + 1)), ("w", Int))
    return Struct(f"gen{seed}", fields)


GEN_SEEDS = list(range(34)) + [35, 47, 129, 149, 180, 298]  # (the last four: identity layouts)


def test_generated_schemas_reach_every_class():
    """Every generated schema is a plan, and together they reach both fixed
    paths, every group KT and tile-eligible and -ineligible programs."""
    paths, kts, tile = set(), set(), set()
    for seed in GEN_SEEDS:
        p = M.Plan(gen_schema(seed))  # raises if xdrg_plan_create refuses it
        assert p.is_fixed
        paths.add(p.path)
        for dec in (0, 1):
            sh = shape(p, dec)
            if sh.grp_G:
                kts.add(sh.grp_KT)
            if p.path == A.PATH_FIXED_LDS:
                tile.add(kernels(p, dec, 1000)[0][0] == "tile")
    assert paths == {A.PATH_FIXED_REG, A.PATH_FIXED_LDS}
    assert kts == {1, 2, 4}
    assert tile == {True, False}


@pytest.mark.parametrize("seed", GEN_SEEDS)
def test_generated_schema_round_trips_on_the_restatement(seed):
    t = gen_schema(seed)
    cp = compile_plan(t)
    nat = make_native(cp, 50, np.random.default_rng(seed))
    x, _ = O.encode(cp, nat, 50)
    back, _ = O.decode(cp, x, 50)
    x2, _ = O.encode(cp, back, 50)
    assert np.array_equal(x, x2)


# ------------------------------------------------------------- case inputs
WIRE_BOOLS = np.array([0, 1, 2, 0x100, 0x80000000], dtype=np.uint32)


def make_native(cp, n, rng):
    """Random native bytes (bool bytes 0..255, padding random); validated
    enums hold tags, since their decode checks them."""
    nat = rng.integers(0, 256, size=(n, cp.stride), dtype=np.uint8)
    for _, k, fl, noff, _, a0, a1 in fields_of(cp):
        if k == A.OP_ENUM and fl & A.F_VALIDATE:
            tags = cp.table[a0:a0 + a1]
            nat[:, noff:noff + 4] = tags[rng.integers(0, a1, size=n)].astype("<u4").view(np.uint8).reshape(n, 4)
    return nat.reshape(-1)


def make_wire(cp, want, n, rng):
    """A valid stream whose bool words are any of WIRE_BOOLS."""
    x = want.reshape(n, cp.fixed_size).copy()
    for _, k, _, _, woff, _, _ in fields_of(cp):
        if k == A.OP_BOOL:
            x[:, woff:woff + 4] = WIRE_BOOLS[rng.integers(0, 5, size=n)].astype(">u4").view(np.uint8).reshape(n, 4)
    return x.reshape(-1)


_cases = {}


def case(t, n, seed=0):
    """(native, its stream, a stream to decode, its records, their stream),
    from the restatement; computed once per layout and batch size."""
    key = (t.name, n, seed)
    if key not in _cases:
        cp = compile_plan(t)
        rng = np.random.default_rng([seed, n, cp.stride])
        nat = make_native(cp, n, rng)
        want, _ = O.encode(cp, nat, n)
        wire = make_wire(cp, want, n, rng)
        back, _ = O.decode(cp, wire, n)
        again, _ = O.encode(cp, back, n)
        for a in (nat, want, wire, back, again):
            a.flags.writeable = False
        if len(_cases) > 64:
            _cases.clear()
        _cases[key] = (nat, want, wire, back, again)
    return _cases[key]


def to_dev(a, dev, shift=0):
    """On the device, 16-byte aligned, or `shift` (4, 8, 12) bytes past it."""
    import torch
    a = np.ascontiguousarray(a)
    if not shift:
        return torch.from_numpy(a.copy()).to(dev)
    big = torch.zeros(a.size + 32, dtype=torch.uint8, device=dev)
    big[shift:shift + a.size] = torch.from_numpy(a.copy()).to(dev)
    return big[shift:shift + a.size]


def run_case(dev, t, opts, n, want_enc=None, want_dec=None, shift=0, seed=0):
    """Encode, decode of a stream with arbitrary bool words, and the encode
    of what that decoded, each exact; the kernels asserted first."""
    import torch
    p = M.Plan(t, opts)
    enc, dec = kernels(p, 0, n, opts, not shift), kernels(p, 1, n, opts, not shift)
    if want_enc is not None:
        assert enc == want_enc, (t.name, n, enc)
    if want_dec is not None:
        assert dec == want_dec, (t.name, n, dec)
    nat, want, wire, back, again = case(t, n, seed)
    mar = M.Marshaler(p, dev)
    s = torch.cuda.current_stream().cuda_stream

    def encode(src):
        out = torch.zeros(n * p.fixed_size + 32, dtype=torch.uint8, device=dev)[shift:shift + n * p.fixed_size]
        assert out.data_ptr() % 16 == shift
        mar.status.init(s)
        mar.launch_encode(to_dev(src, dev, shift), n, out)
        mar.check()
        return out.cpu().numpy()

    def decode(src):
        out = torch.zeros(n * p.stride + 32, dtype=torch.uint8, device=dev)[shift:shift + n * p.stride]
        mar.status.init(s)
        mar.launch_decode(to_dev(src, dev, shift), n, out)
        mar.check()
        return out.cpu().numpy()

    assert np.array_equal(encode(nat), want), (t.name, n, "encode", enc)
    got = decode(wire)
    assert np.array_equal(got, back), (t.name, n, "decode", dec)
    assert np.array_equal(encode(got), again), (t.name, n, "decode->encode", enc)
    return enc, dec


# ======================================================================= GPU
PATHS = {"auto": 0, "lds": 2, "group": 3}


def zoo_ns(p):
    g = max(shape(p, 0).grp_G, shape(p, 1).grp_G, 2)
    return sorted({1, 2, 3, g - 1, g, g + 1, 255, 256, 257, 1000})


def claim(ident, path, n, sh, ks):
    """What a case under fixed_path `path` claims to cover, from the shape of
    its program: the kernels `ks` it ran must be these."""
    checks = bool(sh.has_checks)
    if ident:
        assert ks == [("reg", bool(sh.has_bool), checks, False)]
    elif checks or path == "lds":
        assert ks == [("lds", checks, True)]
    elif path == "auto" and sh.in_words <= 16 and sh.out_words <= 16 and sh.max_terms <= 2:
        assert ks == [("tile", sh.max_terms)]
    elif sh.grp_G and n >= sh.grp_G:
        assert ks[0][:2] == ("grp", sh.grp_KT) and (len(ks) == 2) == bool(n % sh.grp_G)
        assert ks[1:] in ([], [("lds", False, True)])
    else:
        assert ks == [("lds", False, True)]


@gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(ZOO))
def test_zoo_paths_gpu(dev, zoo_gold, name, path):
    """Every zoo layout under every fixed_path: the fixture's 8 records
    first, then random batches around the group size and the tile size."""
    t = ZOO[name]
    opts = {"fixed_path": PATHS[path]}
    p = M.Plan(t, opts)
    e, d = shape(p, 0), shape(p, 1)
    ident = p.path == A.PATH_FIXED_REG
    if path == "group" and not ident and not (e.grp_G or d.grp_G):
        assert name in BIG  # more than 1024 chunks per group: no group program; the LDS kernel
    # the fixture's records: the reference's own bytes
    g = zoo_gold[name]
    mar = M.Marshaler(p, dev)
    nat, x = gold_native(name, g), gold_wire(name, g)
    assert np.array_equal(mar.encode(to_dev(nat, dev), 8).xdr.cpu().numpy(), x)
    want = O.decode(cp_of(name), x, 8)[0] if name in BIG else unhex(g["decoded"])
    assert np.array_equal(mar.decode(to_dev(x, dev), 8)[0].cpu().numpy(), want)
    for n in zoo_ns(p):
        enc, dec = run_case(dev, t, opts, n)
        claim(ident, path, n, e, enc)
        claim(ident, path, n, d, dec)


def test_zoo_covers_the_kernels():
    """What test_zoo_paths_gpu's cases run, from the dispatch rules alone:
    tile with 1 and 2 terms, group with KT 1, 2 and 4 (3-4 terms: bool4's
    and arr5's decode), the LDS kernel with and without checks."""
    seen = set()
    for name, t in ZOO.items():
        for path, fp in PATHS.items():
            p = M.Plan(t, {"fixed_path": fp})
            for n in zoo_ns(p):
                for dec in (0, 1):
                    seen.update(k[:2] if k[0] == "grp" else k for k in kernels(p, dec, n, {"fixed_path": fp}))
    assert {("tile", 1), ("tile", 2), ("grp", 1), ("grp", 2), ("grp", 4), ("lds", False, True),
            ("lds", True, True)} <= seen
    assert {k for k in seen if k[0] == "reg"} == {("reg", b, c, False) for b in (False, True)
                                                  for c in (False, True)}


# ---- register kernel: chunks per record x launch shape
def reg_ns(cpr, fs):
    g0 = cpr // math.gcd(cpr, 256)
    ns = [max(1, 255 // cpr), 256 * g0 // cpr, 256 * g0 // cpr + 1]
    if fs in (0, 3):  # just past the first trip of the 1024 workgroups (rounded up to g0)
        ns.append((1024 + g0 - 1) // g0 * g0 * 256 // cpr + 5)
    return ns


@gpu
@pytest.mark.parametrize("fs", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("name", list(IDENTITY))
def test_reg_shapes(dev, name, fs):
    """k_fixed_reg at 1, 2, 3, 5, 7, 8 and 13 chunks per record under every
    launch shape: fewer chunks than a workgroup, exactly 256 * g0 and one
    past it (g0 = the workgroups a whole number of records take), and for
    the 1024-workgroup shapes a second trip of the grid-stride loop."""
    t = struct_of(name)
    cpr = IDENTITY[name]
    opts = {"fixed_stream": fs}
    p = M.Plan(t, opts)
    e, d = shape(p, 0), shape(p, 1)
    for n in reg_ns(cpr, fs):
        nt, blocks, trips = reg_grid(cpr, n, fs)
        assert nt == (fs in (1, 3)) and blocks % (cpr // math.gcd(cpr, 256)) == 0
        if n == reg_ns(cpr, fs)[-1] and fs in (0, 3):
            assert trips == 2 and blocks >= 1024
        else:
            assert trips == 1
        run_case(dev, t, opts, n, [("reg", bool(e.has_bool), False, nt)],
                 [("reg", bool(d.has_bool), bool(d.has_checks), nt)])


def test_reg_cases_cover_the_instantiations():
    seen = set()
    for name in IDENTITY:
        p = M.Plan(struct_of(name))
        for fs in (-1, 0, 1, 2, 3):
            for dec in (0, 1):
                seen.update(kernels(p, dec, 100, {"fixed_stream": fs}))
    assert seen == {("reg", b, c, nt) for b in (False, True) for c in (False, True) for nt in (False, True)}
    assert sorted(set(IDENTITY.values())) == [1, 2, 3, 5, 7, 8, 13]


# ---- tile kernel: several tiles per workgroup, partial chunks at the end
TILED = ["wide16", "odd7", "numerics", "bool4", "tailbools"]
TILE_NS = (255, 256, 257, 1022, 1023, 1025, 2051)
@gpu
@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("name", TILED)
def test_tile_wrap_and_tails(dev, name, blocks):
    """grp_blocks caps the tile kernel's grid: a workgroup walks several
    tiles and its prefetch runs ahead by the grid size; batch ends whose
    input or output words are no multiple of 4."""
    t = struct_of(name)
    opts = {"grp_blocks": blocks}
    p = M.Plan(t, opts)
    tiled = [dec for dec in (0, 1) if kernels(p, dec, 1000, opts)[0][0] == "tile"]
    assert tiled == ([0] if name == "bool4" else [0, 1])  # (bool4's decode: 4 terms, the group kernel)
    for n in TILE_NS:
        enc, dec = run_case(dev, t, opts, n)
        for prog in tiled:
            assert (enc, dec)[prog] == [("tile", shape(p, prog).max_terms)]


def test_tile_cases_cover_tails_and_terms():
    seen, tails_in, tails_out = set(), set(), set()
    for name in TILED:
        p = M.Plan(struct_of(name))
        for dec in (0, 1):
            ks = kernels(p, dec, 1000)
            if ks[0][0] == "tile":
                seen.add(ks[0])
                sh = shape(p, dec)
                for n in TILE_NS:
                    tails_in.add((n * sh.in_words) % 4)
                    tails_out.add((n * sh.out_words) % 4)
    assert seen == {("tile", 1), ("tile", 2)}
    assert tails_in == {0, 1, 2, 3} and tails_out == {0, 1, 2, 3}
    e = shape(M.Plan(ZOO["wide16"]), 0)
    assert (e.in_words, e.out_words) == (16, 16)


# ---- group kernel
GROUPED = ["numerics", "bool4", "bytes124", "tailbools", "odd7", "wide16", "arr5"]
GRP_OPTS = [{"grp_unroll": u, "grp_nontemporal": nt} for u in (0, 1, 2, 4) for nt in (0, 1)] + \
           [{"grp_blocks": 1}, {"grp_blocks": 7, "grp_nontemporal": 1}]


@gpu
@pytest.mark.parametrize("o", GRP_OPTS, ids=lambda o: "_".join(f"{k[4:]}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", GROUPED)
def test_group_kernel(dev, name, o):
    """k_fixed_grp under fixed_path 3: every KT with each unroll it accepts,
    both store forms, one workgroup, and a workgroup count that has to be
    rounded up to whole groups; batches of one group, 4 groups + 1 record
    (the tail on the LDS kernel) and 4099 records."""
    t = struct_of(name)
    opts = dict(o, fixed_path=3)
    p = M.Plan(t, opts)
    for n in sorted({max(shape(p, 0).grp_G, 1), 4 * shape(p, 0).grp_G + 1, 4099}):
        enc, dec = run_case(dev, t, opts, n)
        for prog, ks in ((0, enc), (1, dec)):
            sh = shape(p, prog)
            assert sh.grp_G
            if sh.has_checks:  # bytes124's decode checks its pads: the LDS kernel
                assert ks == [("lds", True, True)]
                continue
            kt = sh.grp_KT
            u = o.get("grp_unroll", 0) or {1: 4, 2: 2, 4: 1}[kt]
            u = min(u, {1: 4, 2: 2, 4: 1}[kt])
            assert ks[0] == ("grp", kt, u, bool(o.get("grp_nontemporal", 0)))
            assert ks[1:] == ([("lds", False, True)] if n % sh.grp_G else [])


def test_group_cases_cover_the_instantiations():
    seen, tails = set(), set()
    for name in GROUPED:
        for o in GRP_OPTS:
            opts = dict(o, fixed_path=3)
            p = M.Plan(struct_of(name), opts)
            for dec in (0, 1):
                sh = shape(p, dec)
                for n in (sh.grp_G, 4 * sh.grp_G + 1, 4099):
                    ks = kernels(p, dec, n, opts)
                    seen.add(ks[0])
                    if len(ks) == 2:
                        tails.add(sh.grp_G)
                # a workgroup count that is rounded up to whole groups
                if o.get("grp_blocks") == 7 and not sh.has_checks:
                    blocks = min((4099 // sh.grp_G * sh.grp_C + 255) // 256, 7)
                    seen.add(("round", blocks % (sh.grp_C // math.gcd(sh.grp_C, 256)) != 0))
    want = {("grp", kt, u, nt) for kt, us in ((1, (1, 2, 4)), (2, (1, 2)), (4, (1,))) for u in us
            for nt in (False, True)}
    assert want <= seen and ("round", True) in seen
    assert {2, 4} <= tails


# ---- LDS kernel
@gpu
@pytest.mark.parametrize("shift", [0, 4, 8])
@pytest.mark.parametrize("name", list(ZOO))
def test_lds_and_alignment(dev, name, shift):
    """Every zoo layout at 333 records in 16-byte-aligned buffers (under
    fixed_path 2: the LDS kernel's vector form) and in buffers 4 and 8 bytes
    past alignment (every layout then runs its word-by-word form, the
    identity layouts included)."""
    t = ZOO[name]
    opts = {"fixed_path": 2}
    p = M.Plan(t, opts)
    d = shape(p, 1)
    if p.path == A.PATH_FIXED_REG and not shift:
        want_e, want_d = [("reg", bool(d.has_bool), False, False)], [("reg", bool(d.has_bool), bool(d.has_checks), False)]
    else:
        want_e, want_d = [("lds", False, not shift)], [("lds", bool(d.has_checks), not shift)]
    run_case(dev, t, opts, 333, want_e, want_d, shift=shift)


def test_lds_cases_cover_the_instantiations():
    seen = set()
    for name, t in ZOO.items():
        p = M.Plan(t, {"fixed_path": 2})
        for shift in (0, 4):
            for dec in (0, 1):
                seen.update(kernels(p, dec, 333, {"fixed_path": 2}, not shift))
    assert {("lds", c, v) for c in (False, True) for v in (False, True)} <= seen


@gpu
@pytest.mark.parametrize("name", BIG)
def test_big_records_every_route(dev, name):
    """Records of 10 and 20 KB -- a 4-record tile plus the program is 70 and
    140 KB of LDS -- on every route into the LDS kernel: a decode check (any
    decode of these), fixed_path 2, auto, and unaligned buffers."""
    t = ZOO[name]
    for opts, shift in (({}, 0), ({"fixed_path": 2}, 0), ({"fixed_path": 3}, 0), ({}, 4)):
        for n in (1, 5, 64):
            run_case(dev, t, opts, n, [("lds", False, not shift)], [("lds", True, not shift)], shift=shift)


@gpu
@pytest.mark.parametrize("t", [big32k, big36k], ids=lambda t: t.name)
def test_records_that_need_a_smaller_tile(dev, t):
    """32 and 36 KB records: the launcher shrinks the tile to the records
    that fit the workgroup's LDS beside the program (2 and 1 on MI355X)."""
    assert compile_plan(t).fixed_size in (32008, 36004)
    for shift in (0, 4):
        for n in (1, 2, 3, 9):
            run_case(dev, t, {}, n, [("lds", False, not shift)], [("lds", True, not shift)], shift=shift)


@gpu
def test_record_past_the_lds_limit_is_unsupported(dev):
    """A 50 KB record and its program exceed any workgroup's LDS: the launcher
    says so before launching anything (never a failed launch)."""
    p = M.Plan(big50k)
    assert p.path == A.PATH_FIXED_LDS
    mar = M.Marshaler(p, dev)
    nat = to_dev(np.zeros(3 * p.stride, dtype=np.uint8), dev)
    with pytest.raises(A.AbiError, match="EUNSUPPORTED"):
        mar.encode(nat, 3)
    with pytest.raises(A.AbiError, match="EUNSUPPORTED"):
        mar.decode(to_dev(np.zeros(3 * p.fixed_size, dtype=np.uint8), dev), 3)


@gpu
def test_lds_more_tiles_than_workgroups(dev):
    """16,388 records of 8,200 bytes (2,050 words: 4 records per tile) are
    4,097 tiles for the LDS kernel's 4,096 workgroups: the first workgroup
    takes a second tile.  134 MB each way, compared chunk by chunk."""
    import torch
    n, step = 16388, 1024
    p = M.Plan(big8k)
    cp = p.cp
    assert kernels(p, 0, n) == [("lds", False, True)] and kernels(p, 1, n) == [("lds", True, True)]
    assert shape(p, 0).in_words == 2050 and (n + 3) // 4 == 4097
    rng = np.random.default_rng(8200)
    nat = rng.integers(0, 256, size=n * cp.stride, dtype=np.uint8)
    mar = M.Marshaler(p, dev)
    t0 = time.perf_counter()
    res = mar.encode(torch.from_numpy(nat).to(dev), n)
    back, _ = mar.decode(res.xdr, n)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got, back = res.xdr.cpu().numpy(), back.cpu().numpy()
    S_, W = cp.stride, cp.fixed_size
    for r in range(0, n, step):
        m = min(step, n - r)
        want, _ = O.encode(cp, nat[r * S_:(r + m) * S_], m)
        assert np.array_equal(got[r * W:(r + m) * W], want), r
        o_nat, _ = O.decode(cp, want, m)
        assert np.array_equal(back[r * S_:(r + m) * S_], o_nat), r
    print(f"k_fixed_lds wrap: encode+decode of {n} records {1e3 * (t1 - t0):.1f} ms on the device, "
          f"host comparison {time.perf_counter() - t1:.1f} s")


# ---- decode checks
CHECKED = {"id32_mix": ("o", "e"), "id80_enum": ("o", "e2"), "enumpad": ("o", "f")}


@gpu
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("name", list(CHECKED))
def test_decode_checks(dev, zoo_gold, name, shift):
    """1000 records, records 997, 412 and 413 with a nonzero pad byte and 412
    with a word that is no tag in an enum further on: the lowest record and
    its first op in wire order, with the reference's what()
    (k_fixed_reg<., true> aligned for the identity layouts, k_fixed_lds<true, .>
    otherwise)."""
    import torch
    t = ZOO[name]
    p = M.Plan(t)
    cp = p.cp
    n = 1000
    ident = p.path == A.PATH_FIXED_REG and not shift
    d = shape(p, 1)
    assert kernels(p, 1, n, {}, not shift) == ([("reg", bool(d.has_bool), True, False)] if ident
                                               else [("lds", True, not shift)])
    fl = {f[3]: f for f in fields_of(cp)}
    opq, enm = fl[t.offsets[CHECKED[name][0]]], fl[t.offsets[CHECKED[name][1]]]
    assert opq[1] == A.OP_OPAQUE and opq[5] % 4 and enm[1] == A.OP_ENUM and enm[0] > opq[0]
    what = {d_["kind"]: d_["what"] for d_ in zoo_gold[name]["damaged"]}
    x = case(t, n)[1].copy()
    W = cp.fixed_size
    mar = M.Marshaler(p, dev)
    s = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(n * p.stride + 32, dtype=torch.uint8, device=dev)[shift:shift + n * p.stride]

    def verdict(xx):
        mar.status.init(s)
        mar.launch_decode(to_dev(xx, dev, shift), n, out)
        with pytest.raises(M.XdrRuntimeError) as ei:
            mar.check()
        e = ei.value
        with pytest.raises(O.OracleError) as oi:
            O.decode(cp, xx, n)
        assert (e.code, e.record, e.op) == (oi.value.code, oi.value.record, oi.value.op)
        return e

    for r in (997, 412, 413):
        x[r * W + opq[4] + opq[5]] = 0x5a  # the first pad byte
    x[412 * W + enm[4]:412 * W + enm[4] + 4] = (0, 0, 0, 3)
    e = verdict(x)
    assert (e.code, e.record, e.op) == (A.ERR_NONZERO_PAD, 412, opq[0])
    assert type(e) is M.XdrShouldBeZero and str(e) == what["pad"]
    x[412 * W + opq[4] + opq[5]] = 0  # the enum alone in 412
    e = verdict(x)
    assert (e.code, e.record, e.op) == (A.ERR_INVALID_ENUM, 412, enm[0])
    assert type(e) is M.XdrInvariantFailed and str(e) == what["enum"]


@gpu
def test_zoo_capacity_and_length_errors(dev):
    """A short output buffer and a short stream on a zoo layout (arr5, 88
    native and 64 wire bytes): the record and op the restatement names."""
    t = ZOO["arr5"]
    p = M.Plan(t)
    mar = M.Marshaler(p, dev)
    n = 100
    nat, want = case(t, n)[:2]
    cap = 64 * 37 + 20  # record 37 runs out in v[1].b (wire bytes 20..24)
    with pytest.raises(M.XdrOverflow) as ei:
        mar.encode(to_dev(nat, dev), n, capacity=cap)
    assert str(ei.value) == "insufficient buffer space in xdr_generic_put"
    with pytest.raises(O.OracleError) as oi:
        O.encode(p.cp, nat, n, cap=cap)
    assert (ei.value.code, ei.value.record, ei.value.op) == (oi.value.code, oi.value.record, oi.value.op)
    assert (ei.value.record, ei.value.op) == (37, op_at(p.cp, 20))
    xx = want[:64 * 50 + 8].copy()
    with pytest.raises(M.XdrOverflow) as ei:
        mar.decode(to_dev(xx, dev), n)
    with pytest.raises(O.OracleError) as oi:
        O.decode(p.cp, xx, n)
    assert (ei.value.code, ei.value.record) == (oi.value.code, oi.value.record) == (A.ERR_OVERFLOW_GET, 50)


# ---- generated schemas
@gpu
@pytest.mark.parametrize("path", ["auto", "lds"])
@pytest.mark.parametrize("seed", GEN_SEEDS)
def test_generated_schemas_gpu(dev, seed, path):
    """The 40 generated schemas under auto and fixed_path 2, against the
    restatement."""
    t = gen_schema(seed)
    opts = {"fixed_path": PATHS[path]}
    p = M.Plan(t, opts)
    for n in (1, 257, 1000):
        enc, dec = run_case(dev, t, opts, n, seed=seed)
        claim(p.path == A.PATH_FIXED_REG, path, n, shape(p, 0), enc)
        claim(p.path == A.PATH_FIXED_REG, path, n, shape(p, 1), dec)
