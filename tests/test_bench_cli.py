"""bench.py's multi-GPU launch contract, on CPU: `--gpus N` without a distributed
environment starts N ranks itself, and refuses (non-zero exit, before any GPU work)
when fewer than N GPUs are visible. On the GPU: a plain run's result line and --dump-outputs."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def test_bench_refuses_more_gpus_than_visible():
    import torch
    if torch.cuda.device_count() >= 64:
        return
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--gpus 64 but only" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_outputs(tmp_path):
    """A plain run on 3 blocks (12 MiB: above DUMP_SAMPLE, so the sampled dump): the result line has
    the headline fields and none of the --full legs, and --dump-outputs holds the last step's
    outputs: the decoded bytes at the seeded positions, lengths, statuses and per-block XXH32,
    all equal to the CPU oracle's generator for the bench's seeds (1 + block)."""
    import importlib.util
    import json
    import numpy as np
    import oracle as O
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--blocks", "3", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["unit"] == "GB/s" and line["dtype"] == "u8" and line["higher_is_better"] is True
    assert line["metric"] == bench.METRIC and line["ms_per_step"] > 0
    assert abs(line["value"] - 3 * bench.BLOCK / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.011 * max(1.0, line["value"])
    for k in ("compress", "roundtrip_GBps", "reference_mode", "variants", "latency_curve", "frame", "single_block",
              "napi_end_to_end", "reference_benchmark", "cpu_baseline", "cpu_baseline_c_oracle"):
        assert k not in line, k
    B = bench.BLOCK
    raw = np.concatenate([O.generate("tiles216", 1 + b, B) for b in range(3)])
    pos = np.sort(np.random.default_rng(0x5EED).integers(0, raw.size, bench.DUMP_SAMPLE))
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["decoded", "decoded_len", "decoded_xxh32", "status"]
    assert got["decoded"].dtype == np.float32 and np.array_equal(got["decoded"], raw[pos].astype(np.float32))
    assert np.array_equal(got["decoded_len"], np.full(3, B, np.float32))
    assert np.array_equal(got["status"], np.zeros(3, np.float32))
    assert got["decoded_xxh32"].dtype == np.float64
    assert [int(x) for x in got["decoded_xxh32"]] == [O.xxh32(raw[b * B:(b + 1) * B]) for b in range(3)]
