"""tests/golden/sort.json (tests/golden/make_sort.py): the fixture
regenerates, and the Python model of xdrg_compare (tests/compare_model.py)
orders every pool as the reference's std::stable_sort / std::unique did --
with the claim xdrg_sort rests on checked on real values: every pair of
sortable pool members compares less, equivalent or greater."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import compare_model as CM
import sort_fixture as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REF", "/root/reference")


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "xdrpp", "marshal.cc")), reason="the reference tree is absent")
def test_fixture_regenerates(tmp_path):
    out = str(tmp_path / "sort.json")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_sort.py"), out], check=True,
                   capture_output=True)
    with open(out, "rb") as f, open(F.PATH, "rb") as g:
        assert f.read() == g.read()


def test_fixture_is_not_thin():
    assert os.path.getsize(F.PATH) < 200_000
    for name in F.TYPES:
        p = F.pool(name)
        assert p.n == 64 and p.m >= 48, name
        assert p.m - p.distinct >= 8, name  # values with an equivalent earlier one
        ident = np.sort(p.sorted)
        assert not np.array_equal(p.sorted, ident) and not np.array_equal(p.sorted, ident[::-1]), name
        assert len(p.unsortable) >= (2 if name in F.FLOAT_TYPES else 0), name
        t = F.raw()[name]
        assert 2 * t["altered_dropped"] <= t["altered_tried"], name
        assert sorted(p.perm.tolist()) == list(range(p.n)), name


@functools.lru_cache(maxsize=None)
def _matrix(name):
    """The model's pool[i] <=> pool[j] for every i, j."""
    p = F.pool(name)
    st = p.cp.stride
    rows = p.nat.reshape(p.n, st)
    i, j = np.divmod(np.arange(p.n * p.n), p.n)
    got = CM.compare(p.cp, rows[i].reshape(-1), p.heap, rows[j].reshape(-1), p.heap, p.n * p.n)
    return got.reshape(p.n, p.n)


@pytest.mark.parametrize("name", list(F.TYPES))
def test_model_self_compare_gives_unsortable(name):
    p = F.pool(name)
    assert np.array_equal(np.nonzero(np.diag(_matrix(name)) != CM.EQUAL)[0], p.unsortable)


@pytest.mark.parametrize("name", list(F.TYPES))
def test_sortable_members_are_totally_ordered(name):
    p = F.pool(name)
    sub = _matrix(name)[np.ix_(p.sorted, p.sorted)]
    assert np.isin(sub, [CM.LESS, CM.EQUAL, CM.GREATER]).all()
    assert np.array_equal(sub, -sub.T)  # antisymmetric, equivalence symmetric


@pytest.mark.parametrize("name", list(F.TYPES))
def test_model_orders_the_pool_as_recorded(name):
    p = F.pool(name)
    M = _matrix(name)

    def cmp(a, b):
        return -1 if M[a, b] == CM.LESS else 1 if M[b, a] == CM.LESS else a - b  # the index breaks a tie

    ok = [i for i in range(p.n) if M[i, i] == CM.EQUAL]
    got = sorted(ok, key=functools.cmp_to_key(cmp))
    assert got == p.sorted.tolist()
    first = [int(k == 0 or M[got[k - 1], got[k]] == CM.LESS) for k in range(len(got))]
    assert first == p.first.tolist()
