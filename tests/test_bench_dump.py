"""bench.py's plain run and --dump-outputs.

A plain run (no --full) only sets up, warms up, times --steps steps and
prints the line: none of the legs beside the headline appear in it.
--dump-outputs DIR writes what the last timed step computed as float32 /
float64 .npy files; the inputs are seeded, so the files must equal the
oracle's encoding of the same batch (CPU stand-in engine) or the golden
fixtures (GPU engine) element for element.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

import oracle_bridge as O
from xdrpp_amd import schemas as S
from xdrpp_amd import shard as SH
from xdrpp_amd import workloads as W
from xdrpp_amd.xdr_types import compile_plan

FULL_ONLY = ("large_batch_16m", "shard_2m", "cold_cache", "plain_stream", "messages", "rpc_headers",
             "host_inclusive", "cpu_baseline", "gather")


def run_bench(extra, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path)] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * line["config"]["xdr_bytes_per_gpu"] / 2**30 /
                                          (line["ms_per_step"] * 1e-3), rel=0.01, abs=0.01)
    assert line["round_trip_ok"] is None and line["bit_exact_vs_reference"] is None
    assert not [k for k in FULL_ONLY if k in line]
    return line


def test_plain_run_dumps_outputs_cpu_engine(tmp_path):
    n, schema = 700, "recvar"
    run_bench(["--records", str(n), "--schema", schema,
               "--engine", os.path.join(ROOT, "tests", "bench_cpu_engine.py")], tmp_path)
    cp = compile_plan(S.ALL[schema])
    nat, heap = W.GENERATORS[schema](n, seed=SH.seed_for(schema, 1))
    want, woffs = O.encode(cp, nat, n, heap)
    wnat, wheap = O.decode(cp, want, n, woffs)
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["decoded_heap", "decoded_native", "offsets", "xdr"]
    assert got["xdr"].dtype == np.float32 and got["offsets"].dtype == np.float64
    assert np.array_equal(got["xdr"], want.astype(np.float32))
    assert np.array_equal(got["offsets"], woffs.view(np.int64).astype(np.float64))
    assert np.array_equal(got["decoded_native"], wnat.view(np.uint8).astype(np.float32))
    assert np.array_equal(got["decoded_heap"], wheap.view(np.uint8).astype(np.float32))


def test_dump_sample_is_fixed_and_capped():
    torch = pytest.importorskip("torch")
    import bench
    t = torch.arange(10 * bench.DUMP_BLOCK + 123, dtype=torch.int64)
    whole = bench.dump_sample(t, 8 * t.numel(), 1)
    assert whole.dtype == np.float64 and np.array_equal(whole, t.numpy().astype(np.float64))
    budget = 8 * 4 * bench.DUMP_BLOCK  # four blocks of the eleven
    a, b = bench.dump_sample(t, budget, 1), bench.dump_sample(t, budget, 1)
    assert np.array_equal(a, b) and a.nbytes <= budget
    assert a.size == 3 * bench.DUMP_BLOCK + 123  # the last block is the short one
    assert a[0] == 0 and a[-1] == t.numel() - 1 and np.all(np.diff(a) > 0)
    u8 = (t % 251).to(torch.uint8)
    s = bench.dump_sample(u8, 4 * 4 * bench.DUMP_BLOCK, 1)
    assert s.dtype == np.float32 and np.array_equal(s, (a % 251).astype(np.float32))


def test_legs_beside_the_headline_need_full():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--msgs"], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 2 and "--full" in out.stderr


@pytest.mark.gpu
def test_plain_run_dumps_outputs_gpu(dev, tmp_path):
    n = 1024
    line = run_bench(["--records", str(n)], tmp_path)
    assert line["roofline"]["kernel"] == "k_fixed_reg"
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["decoded_native", "xdr"]
    assert got["xdr"].dtype == np.float32 and got["decoded_native"].dtype == np.float32
    assert np.array_equal(got["xdr"], golden("rec128", n, "xdr").astype(np.float32))
    assert np.array_equal(got["decoded_native"], golden("rec128", n, "native").astype(np.float32))
