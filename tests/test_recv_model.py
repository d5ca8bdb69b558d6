"""CPU: the host model of the receive batch (tests/recv_model.py) held to the
reference: tests/golden/recv.json is what the REAL read_message with
msg_sock's length rule gives every connection of a seeded set (script
tests/golden/make_recv.py), tests/golden/frames.json what it gives the long
streams of tests/msg_streams.py, each taken here as one connection.

    `what` from the reference            model
    null                                 OPEN, need 0
    premature EOF                        OPEN, consumed = last offset, need from the bytes
    message fragments unimplemented      FRAGMENT
    too long                             TOO_LONG

BAD_SIZE and BAD_RPC have no reference binary behind them: read_message has
the pre-swap size test (srpc.cc:38-39) but none of the fixtures' sizes trip
it, msg_sock::input has no size test at all, and the oracle does not run
rpc_sock::recv_msg.  They are pinned to the cited lines only (srpc.cc:38-39,
marshal.h:152-162, msgsock.cc:205-224).  No GPU."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD

import msg_streams as MS
import recv_model as RM

WHAT_STATE = {None: RM.OPEN, "read_message: premature EOF": RM.OPEN,
              "read_message: message fragments unimplemented": RM.FRAGMENT, "too long": RM.TOO_LONG}


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLD, "recv.json")) as f:
        return json.load(f)


def fixture_bytes(c) -> np.ndarray:
    return RM.connection(c["seed"], c["sizes"], c["edits"].get("frag"), c["edits"].get("cut", 0))


def need_from_bytes(x: np.ndarray, at: int) -> int:
    """What the tail x[at:] must grow to: 4 inside the mark, 4 + size inside the body."""
    if x.size - at < 4:
        return 4 if x.size > at else 0
    return 4 + (int.from_bytes(x[at:at + 4].tobytes(), "big") & 0x7FFFFFFF)


def hold(x: np.ndarray, maxlen: int, offsets, what):
    msgs, consumed, need, state = RM.frame(x, maxlen)
    assert [p for p, _, _ in msgs] + [consumed] == offsets
    assert state == WHAT_STATE[what]
    if what is None:
        assert need == 0 and consumed == x.size
    elif state == RM.OPEN:
        assert consumed < x.size and need == need_from_bytes(x, consumed) and need > x.size - consumed
    else:
        assert need == 0
    return msgs, consumed, need, state


def test_fixture_bytes_and_coverage(fixture):
    cs = fixture["connections"]
    assert 35 <= len(cs) <= 48 and fixture["max_msg_len"] == 4096
    tails = set()
    for c in cs:
        x = fixture_bytes(c)
        assert x.size == c["bytes"] and MS.sha256(x) == c["sha256"], c["seed"]
        assert all(s % 4 == 0 for s in c["sizes"])
        if c["what"] == "read_message: premature EOF":
            tails.add(min(x.size - c["offsets"][-1], 4))
    assert tails == {1, 2, 3, 4}                        # inside a mark (1, 2, 3 bytes) and inside a body
    whats = [c["what"] for c in cs]
    assert all(whats.count(w) >= 4 for w in WHAT_STATE)
    assert sum(c["bytes"] == 0 for c in cs) >= 2 and any(0 in c["sizes"] for c in cs)
    frag_at = {(c["edits"]["frag"], len(c["sizes"])) for c in cs if "frag" in c["edits"]}
    assert any(k == 0 for k, n in frag_at) and any(0 < k < n - 1 for k, n in frag_at) and \
        any(k == n - 1 for k, n in frag_at)
    m = fixture["max_msg_len"]
    for size in (m, m + 4):  # with and without the body present
        assert any(size in c["sizes"] and not c["edits"] for c in cs)
        assert any(size in c["sizes"] and c["edits"].get("cut", 0) >= size for c in cs)


def test_model_on_the_fixture(fixture):
    for c in fixture["connections"]:
        hold(fixture_bytes(c), fixture["max_msg_len"], c["offsets"], c["what"])


def test_model_on_the_long_streams():
    with open(os.path.join(GOLD, "frames.json")) as f:
        frames = json.load(f)
    cache = {}
    for fr in frames["framings"]:
        name = fr["stream"]
        if name not in cache:
            cache[name] = MS.stream(name)
            assert MS.sha256(cache[name]) == frames["streams"][name]["sha256"]
        _, consumed, need, state = hold(cache[name], fr["max_msg_len"], fr["offsets"], fr["what"])
        if name == "trunc_long":  # a cut tail is no error here
            assert state == RM.OPEN and need == 4 + MS.MIB


def test_batch_of_the_fixture(fixture):
    """The batch is the connections side by side: first is the exclusive scan
    of msgs, the stream the concatenation of the consumed prefixes."""
    xs = [fixture_bytes(c) for c in fixture["connections"]]
    buf, segs = RM.pack(xs)
    stream, offsets, conn_of, kind, conns = RM.recv_batch(buf, segs, fixture["max_msg_len"])
    assert np.array_equal(conns["first"], np.concatenate([[0], np.cumsum(conns["msgs"])[:-1]]))
    assert offsets.size == conn_of.size + 1 == int(conns["msgs"].sum()) + 1
    assert offsets[-1] == stream.size == int(conns["consumed"].sum())
    for c, (x, rec) in enumerate(zip(xs, conns)):
        f, n = int(rec["first"]), int(rec["msgs"])
        assert (conn_of[f:f + n] == c).all()
        assert np.array_equal(stream[int(offsets[f]):int(offsets[f + n])], x[:int(rec["consumed"])])
        assert [int(o - offsets[f]) for o in offsets[f:f + n + 1]] == fixture["connections"][c]["offsets"]
    assert not kind.any()


def test_bad_size_and_bad_rpc_by_the_cited_lines():
    rng = np.random.default_rng(5)
    good = RM.message(rng, 8, word1=0)
    # srpc.cc:38-39: the first byte of the mark, before the swap
    m = RM.message(rng, 8)
    m[0] |= 1
    assert RM.frame(np.concatenate([good, m]))[1:] == (12, 0, RM.BAD_SIZE)
    # marshal.h:152-162: a size that is not a multiple of 4 -- open until the body is there
    m = RM.message(rng, 10)
    assert RM.frame(np.concatenate([good, m[:9]]))[1:] == (12, 14, RM.OPEN)
    assert RM.frame(np.concatenate([good, m]))[1:] == (12, 0, RM.BAD_SIZE)
    # the order of ix_mark's tests: the size test before the fragment bit, the fragment bit before the length
    m = RM.message(rng, 8, frag=True)
    m[0] |= 2
    assert RM.frame(m)[3] == RM.BAD_SIZE
    m = RM.message(rng, 0x200000, frag=True)[:4]
    assert RM.frame(m)[3] == RM.FRAGMENT
    # msgsock.cc:205-224: shorter than 8 bytes, word 1 neither CALL nor REPLY
    for bad in (RM.message(rng, 0), RM.message(rng, 4), RM.message(rng, 8, word1=2),
                RM.message(rng, 12, word1=0x01000000)):
        msgs, consumed, need, state = RM.frame(np.concatenate([good, bad, good]), rpc=True)
        assert (len(msgs), consumed, need, state) == (1, 12, 0, RM.BAD_RPC)
        assert RM.frame(np.concatenate([good, bad, good]))[3] == RM.OPEN  # without the flag no such test
    msgs, _, _, state = RM.frame(np.concatenate([good, RM.message(rng, 40, word1=1)]), rpc=True)
    assert [k for _, _, k in msgs] == [0, 1] and state == RM.OPEN
    # a cut message is not judged before it is whole
    assert RM.frame(RM.message(rng, 8, word1=7)[:11], rpc=True)[1:] == (0, 12, RM.OPEN)
