"""The value classes the C++ layer records (include/xdrpp_gpu.hh:
record_type / record_union, from std::is_floating_point_v / is_signed_v of
the field types and the unions' declared discriminant types) against the
Python mirror's, op for op, on the reference's genuine xdrc-generated types.
tests/cpp/compare_classes.cc is compiled here against the generated headers
(`make -C oracle`) and the reference tree; skipped where they are absent."""
import os
import subprocess

import pytest

import compare_fixture as F
from xdrpp_amd import build as B
from xdrpp_amd.xdr_types import compile_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "oracle", "_ref", "gen", "inc")
REF = os.environ.get("REF", "/root/reference")
LIBDIR = os.path.join(ROOT, "xdrpp_amd")

pytestmark = pytest.mark.skipif(
    not (os.path.exists(os.path.join(INC, "tests", "xdrtest.hh")) and os.path.exists(os.path.join(INC, "kat.hh"))
         and os.path.exists(os.path.join(REF, "xdrpp", "marshal.cc"))),
    reason="oracle/_ref/gen/inc or the reference tree is absent")


def test_cpp_classes_equal_the_python_mirror(tmp_path):
    exe = str(tmp_path / "compare_classes")
    subprocess.run([B.hipcc(), "-std=c++20", "-O1", "-DXDRPP_WORDS_BIGENDIAN=0", "-I", INC, "-I", REF,
                    "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "compare_classes.cc"), os.path.join(REF, "xdrpp", "marshal.cc"),
                    "-L", LIBDIR, "-lxdrgpu", f"-Wl,-rpath,{LIBDIR}"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    got, cur = {}, None
    for line in out:
        w = line.split()
        if w and w[0] == "type":
            cur = got.setdefault(w[1], [])
        elif w:
            cur.append((int(w[0]), int(w[1])))
    assert sorted(got) == sorted(F.TYPES)
    for name, t in F.TYPES.items():
        cp = compile_plan(t)
        want = list(zip((int(k) for k in cp.ops["kind"]), (int(c) for c in cp.cmp_classes)))
        assert got[name] == want, name
