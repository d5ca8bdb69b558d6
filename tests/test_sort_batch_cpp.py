"""xdr::gpu::sort_batch / sort_workspace_size (include/xdrpp_gpu.hh) on the
reference's genuine xdrc-generated types: tests/cpp/sort_batch.cc is
compiled here against the generated headers (`make -C oracle`) and the
reference tree and linked with the library, and its host-check paths run (a
null batch throws the XDRG_EINVAL exception, n = 0 returns); no device is
touched.  Skipped where the headers or the reference tree are absent."""
import os
import subprocess

import pytest

from xdrpp_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "oracle", "_ref", "gen", "inc")
REF = os.environ.get("REF", "/root/reference")
LIBDIR = os.path.join(ROOT, "xdrpp_amd")

pytestmark = pytest.mark.skipif(
    not (os.path.exists(os.path.join(INC, "tests", "xdrtest.hh")) and os.path.exists(os.path.join(INC, "kat.hh"))
         and os.path.exists(os.path.join(REF, "xdrpp", "marshal.cc"))),
    reason="oracle/_ref/gen/inc or the reference tree is absent")


def test_sort_batch_instantiates_and_checks_its_arguments(tmp_path):
    exe = str(tmp_path / "sort_batch")
    subprocess.run([B.hipcc(), "-std=c++20", "-O1", "-DXDRPP_WORDS_BIGENDIAN=0", "-I", INC, "-I", REF,
                    "-I", os.path.join(ROOT, "oracle"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "sort_batch.cc"), os.path.join(REF, "xdrpp", "marshal.cc"),
                    "-L", LIBDIR, "-lxdrgpu", f"-Wl,-rpath,{LIBDIR}"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [w for w in out if w.startswith("ok ")] == ["ok numerics", "ok containertest", "ok rp__list"]
    assert sum("xdrg_sort failed (-1)" in w for w in out) == 3
