"""GPU: bench.py on one GPU, plain and with --full.  A plain run measures the headline and nothing else (no untimed pass of the
kernels alone, no CPU baseline, on the N > 1 code path no second split of the GPUs); --full adds them to the same JSON line."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def bench_line(*extra, launcher=(), env=None):
    cmd = [sys.executable] + list(launcher) + [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                                               "--ppd", "256"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "particles/sec (grid->displacements)" and d["unit"] == "particles/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 1e7
    assert abs(d["ms_per_step"] - 256.0 ** 3 / d["value"] * 1e3) <= 1e-9 * d["ms_per_step"]
    assert d["kernels"]["k_xfft"]["ms_per_step"] > 0 and d["roofline"]["frac"] > 0  # from the timed steps: in both kinds of run
    return d


def test_plain_run_measures_the_headline_only():
    d = bench_line()
    assert d["kernels_isolated"] is None and "cpu_baseline" not in d and "modes" not in d


def test_full_run_adds_the_isolated_pass_and_the_cpu_baseline():
    d = bench_line("--full")
    assert d["kernels_isolated"]["k_yfft"]["ms_per_step"] > 0 and d["kernels_isolated"]["k_xfft"]["ms_per_step"] > 0
    cb = d["cpu_baseline"]
    assert cb["value"] is not None and cb["value"] > 0 and cb["ppd"] <= 256 and cb["kind"] == "port", cb


def test_plain_run_on_the_distributed_code_path_times_the_default_split_only():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    d = bench_line("--dist", env=env, launcher=("-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                                                "--master-addr", "127.0.0.1", "--master-port", "29537"))
    m = d["modes"]
    assert set(m) == {"default", m["default"], "link_probe", "estimate_at_probed_rate"}, m
    assert abs(m[m["default"]]["particles_per_s"] - d["value"]) <= 1e-9 * d["value"] and len(d["per_rank"]) == 1
    assert d["kernels_isolated"] is None and "cpu_baseline" not in d
