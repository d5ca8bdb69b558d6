"""Regenerate tests/golden/sort.json: what std::stable_sort and std::unique
give with the REAL operator< (xdrpp/types.h:946-1062, XDRPP_STRONG_ORDER = 0)
on pools of 64 values of the genuine xdrc-generated types --
tests/cpp/sort_ref.cc, compiled here against the generated headers
(`make -C oracle`) and the reference's marshal.cc into a temporary directory;
nothing compiled is kept.  The program refuses to write a thin fixture (48
sortable values a type, 8 with an equivalent earlier one, an order that is
neither the identity nor its reverse, 2 unsortable values for the float types,
at most half of the altered candidates dropped).  Test infrastructure.

    python tests/golden/make_sort.py [OUT.json]
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(ROOT, "oracle")
REF = os.environ.get("REF", "/root/reference")
INC = os.path.join(ORACLE, "_ref", "gen", "inc")
HEADERS = ["tests/xdrtest.hh", "xdrpp/rpc_msg.hh", "xdrpp/rpcb_prot.hh", "bench.hh", "validated.hh", "kat.hh"]


def main(dest: str) -> None:
    subprocess.run(["make", "-s", "-C", ORACLE, f"REF={REF}"] + [f"_ref/gen/inc/{h}" for h in HEADERS], check=True)
    with tempfile.TemporaryDirectory() as td:
        exe, out = os.path.join(td, "sort_ref"), os.path.join(td, "sort.json")
        subprocess.run(["g++", "-I", INC, "-I", REF, "-I", ORACLE, "-I", os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "sort_ref.cc"),
                        os.path.join(REF, "xdrpp", "marshal.cc"), "-std=c++20", "-O2",
                        "-DXDRPP_WORDS_BIGENDIAN=0"], check=True)
        subprocess.run([exe, out], check=True)
        with open(out, "rb") as f:
            data = f.read()
    with open(dest, "wb") as f:
        f.write(data)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sort.json"))
