"""Regenerate tests/golden/recv.json: the framing the REAL read_message with
msg_sock's length rule (oracle/_ref/ref_golden frame, built by `make -C
oracle`) gives each connection of a seeded set of receive buffers -- whole
messages, tails cut inside a mark and inside a body, segments that end at a
mark, cleared fragment bits, sizes at and past max_msg_len with and without
their bodies, empty messages, empty segments.  All sizes are multiples of 4,
so read_message and xdrg_rpc_recv_batch agree on the chain.  Test
infrastructure.

    python tests/golden/make_recv.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import msg_streams as MS  # noqa: E402
import recv_model as RM  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_golden")
MAXLEN = 4096

# (sizes, edits): frag = message whose mark loses the last-fragment bit, cut = bytes dropped from the end
CASES = [
    # whole messages; the segment ends exactly at a mark
    ([8], {}), ([8, 8, 8], {}), ([100, 8, 0, 40], {}), ([44] * 5, {}), ([8] * 100, {}), ([1016], {}), ([1020], {}),
    ([1024], {}), ([200] * 10, {}),
    # empty messages, empty segments
    ([0], {}), ([0, 0, 0], {}), ([0, 8, 0], {}), ([], {}), ([], {}),
    # tails cut inside a mark: 1, 2 and 3 bytes of it are there
    ([8, 8, 8], {"cut": 11}), ([8, 8, 8], {"cut": 10}), ([8, 8, 8], {"cut": 9}),
    ([8], {"cut": 11}), ([8], {"cut": 10}), ([8], {"cut": 9}), ([8] * 100, {"cut": 10}),
    # tails cut inside a body
    ([8, 100], {"cut": 50}), ([8, 100], {"cut": 100}), ([40], {"cut": 39}), ([40], {"cut": 1}),
    ([8] * 100, {"cut": 5}), ([0, 0, 8], {"cut": 8}),
    # a cleared fragment bit in the first, a middle and the last message; with the mark alone
    ([8, 8, 8], {"frag": 0}), ([8, 16, 8, 8], {"frag": 2}), ([8, 8, 8], {"frag": 2}), ([8, 8], {"frag": 1, "cut": 8}),
    ([200] * 10, {"frag": 7}), ([0, 0], {"frag": 1}),
    # sizes at max_msg_len and 4 above it, with and without the body
    ([4096], {}), ([8, 4096, 8], {}), ([8, 4096], {"cut": 4096}), ([8, 4096], {"cut": 1}),
    ([8, 4100], {}), ([8, 4100], {"cut": 4100}), ([8, 4100], {"cut": 4000}), ([4100, 8], {}),
]


def main() -> None:
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/ref_golden"], check=True)
    out = {"generator": "oracle/ref_golden frame (read_message, srpc.cc:29-55, with msg_sock's maxmsglen rule, "
                        "msgsock.cc:97-111) on each connection of tests/golden/make_recv.py; bytes: "
                        "recv_model.connection(seed, sizes, frag, cut)",
           "max_msg_len": MAXLEN, "connections": []}
    with tempfile.TemporaryDirectory() as td:
        for i, (sizes, edits) in enumerate(CASES):
            seed = 7000 + i
            x = RM.connection(seed, sizes, edits.get("frag"), edits.get("cut", 0))
            path, res = os.path.join(td, "c"), os.path.join(td, "r.json")
            x.tofile(path)
            subprocess.run([REF, "frame", path, str(MAXLEN), res], check=True)
            with open(res) as f:
                r = json.load(f)
            out["connections"].append({"seed": seed, "sizes": sizes, "edits": edits, "bytes": int(x.size),
                                       "sha256": MS.sha256(x), **r})
    with open(os.path.join(HERE, "recv.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
