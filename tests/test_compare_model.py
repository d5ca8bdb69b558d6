"""The Python model of xdrg_compare (tests/compare_model.py) against the
reference's recorded operator<=> / operator== (tests/golden/compare.json,
tests/golden/make_compare.py): every pair of every type, operands decoded by
the C restatement."""
import numpy as np
import pytest

import compare_fixture as F
import compare_model as CM


def test_fixture_is_not_thin():
    for name in F.TYPES:
        t = F.raw()[name]
        cmp = [p[3] for p in t["pairs"]]
        assert len(cmp) >= 64, name
        for v in (-1, 0, 1) + ((2,) if name in F.FLOAT_TYPES else ()):
            assert cmp.count(v) >= 4, (name, v)
        assert 2 * t["altered_dropped"] <= t["altered_tried"], name


@pytest.mark.parametrize("name", list(F.TYPES))
def test_eq_is_equivalent(name):
    b = F.batch(name)
    assert np.array_equal(b.eq, b.cmp == 0)


@pytest.mark.parametrize("name", list(F.TYPES))
def test_model_equals_reference(name):
    b = F.batch(name)
    got = CM.compare(b.cp, b.nat_a, b.heap_a, b.nat_b, b.heap_b, b.n)
    bad = np.nonzero(got != b.cmp)[0]
    assert bad.size == 0, (name, [(int(i), b.how[i], int(got[i]), int(b.cmp[i])) for i in bad[:8]])


def test_model_void_and_unknown_arms_compare_equal():
    # equal discriminants that select no arm at all: equivalent, and the walk goes on behind the union
    from xdrpp_amd.xdr_types import Int, Struct, compile_plan
    t = Struct("t", [("u", F.ContainsEnum), ("x", Int)])
    cp = compile_plan(t)
    a = np.zeros(cp.stride, dtype=np.uint8)
    a[0] = 7  # no such case, no default
    b = a.copy()
    assert CM.compare(cp, a, None, b, None, 1)[0] == CM.EQUAL
    b[t.offsets["x"]] = 1
    assert CM.compare(cp, a, None, b, None, 1)[0] == CM.LESS
