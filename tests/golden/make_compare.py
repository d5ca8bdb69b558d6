"""Regenerate tests/golden/compare.json: what the REAL operator<=> and
operator== (xdrpp/types.h:946-1062, XDRPP_STRONG_ORDER = 0) give seeded
pairs of the genuine xdrc-generated types -- tests/cpp/compare_ref.cc,
compiled here against the generated headers (`make -C oracle`) and the
reference's marshal.cc into a temporary directory; nothing compiled is kept.
The program refuses to write a thin fixture (64 pairs a type, every result 4
times, at most half of the altered candidates dropped).  Test infrastructure.

    python tests/golden/make_compare.py
"""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(ROOT, "oracle")
REF = os.environ.get("REF", "/root/reference")
INC = os.path.join(ORACLE, "_ref", "gen", "inc")
HEADERS = ["tests/xdrtest.hh", "xdrpp/rpc_msg.hh", "xdrpp/rpcb_prot.hh", "bench.hh", "validated.hh", "kat.hh"]


def main() -> None:
    subprocess.run(["make", "-s", "-C", ORACLE, f"REF={REF}"] + [f"_ref/gen/inc/{h}" for h in HEADERS], check=True)
    with tempfile.TemporaryDirectory() as td:
        exe, out = os.path.join(td, "compare_ref"), os.path.join(td, "compare.json")
        subprocess.run(["g++", "-I", INC, "-I", REF, "-I", ORACLE, "-I", os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "compare_ref.cc"),
                        os.path.join(REF, "xdrpp", "marshal.cc"), "-std=c++20", "-O2",
                        "-DXDRPP_WORDS_BIGENDIAN=0"], check=True)
        subprocess.run([exe, out], check=True)
        os.replace(out, os.path.join(HERE, "compare.json"))


if __name__ == "__main__":
    main()
