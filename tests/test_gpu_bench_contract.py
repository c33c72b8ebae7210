"""bench.py contract on the GPU box: one JSON line with the required keys at N = 1, and the N = 2 code path (site partition x2,
max-over-ranks timing, packed all-reduce of the results) rehearsed with two ranks sharing the one GPU over gloo
(BENCH_REHEARSAL=1; on the 8-GPU node the same code runs over RCCL with one rank per device)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "roofline"}


def last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def test_bench_single_gpu_small():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--sites", "8", "--cells", "10", "--lld", "12",
                        "--no-green", "--full"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = last_json(r.stdout)
    assert REQUIRED <= set(d) and "cpu_baseline" in d
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["dtype"] == "f64" and d["scaling"] == "weak" and d["vs_baseline"] is None
    rf = d["roofline"]
    # fractions are quoted in the flops the operator's block structure requires: a kernel cannot beat the pipe's peak in them
    assert d["value"] > 0 and rf["bound"] == "mfma" and 0 < rf["frac"] <= 1 and 0 < rf["frac_step"] <= 1
    assert rf["frac"] <= rf["frac_algorithmic"] and 0.5 <= rf["required_per_algorithmic"] <= 1.0      # collinear bcc Fe: 14 of 15 blocks spin-diagonal
    assert d["cpu_baseline"]["kind"] in ("reference", "port") and d["cpu_baseline"]["value"] > 0


def test_bench_two_ranks_rehearsal():
    """`bench.py --gpus 2` with no launcher around it: the script starts its two ranks itself (BENCH_REHEARSAL: they share the box's
    one GPU and reduce over gloo; on a multi-GPU node the same command runs one rank per device over RCCL)."""
    env = dict(os.environ, BENCH_REHEARSAL="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--sites", "8", "--cells", "10", "--lld", "12",
           "--master-port", "29533"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = last_json(r.stdout)
    assert REQUIRED <= set(d)
    assert d["n_gpus"] == 2 and "x2" in d["config"]["parallelism"] and d["value"] > 0
    assert "cpu_baseline" not in d                    # CPU leg on rank 0 at N = 1 only
    assert "gloo" in d["config"]["collective"]


def test_bench_refuses_world_size_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and "refusing" in r.stderr


def test_bench_step_fractions():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--sites", "8", "--cells", "10", "--lld", "12",
                        "--no-green", "--no-cpu", "--recur", "chebyshev"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = last_json(r.stdout)
    rf = d["roofline"]
    assert abs(rf["frac_step_algorithmic"] - d["value"] * 1e-3 / d["n_gpus"] / rf["peak"]) < 1e-9 and rf["frac"] == rf["frac_kernel"]
    assert 0 < rf["frac_step"] <= rf["frac_step_algorithmic"] and rf["frac_step"] <= 1
    assert "Chebyshev" in d["config"]["workload"]


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run prints the headline line only (the LDOS stage and the CPU baseline sit behind --full), times exactly --steps steps,
    and --dump-outputs writes the coefficients the last timed step returned: the CPU oracle's on the same sites."""
    import importlib.util
    import numpy as np
    from helpers import RTOL, rel_err
    from oracle import oracle
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--sites", "8", "--cells", "10", "--lld", "12",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = last_json(r.stdout)
    assert REQUIRED <= set(d) and "cpu_baseline" not in d and "ldos" not in d
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    # the launches counted inside the timed loop follow --steps: twice those of a one-step run
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--sites", "8", "--cells", "10", "--lld", "12"],
                        capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r1.returncode == 0, r1.stderr[-2000:]
    launches1 = last_json(r1.stdout)["roofline"]["launches"]
    assert launches1 > 0 and d["roofline"]["launches"] == 2 * launches1, (d["roofline"]["launches"], launches1)
    assert sorted(os.listdir(out)) == ["a_b.npy", "b2_b.npy"]
    a, b2 = np.load(out / "a_b.npy"), np.load(out / "b2_b.npy")
    assert a.dtype == b2.dtype == np.float64 and a.shape == b2.shape == (18, 18, 12, 8, 2)
    spec = importlib.util.spec_from_file_location("bench_dump", os.path.join(ROOT, "bench.py"))
    bm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bm)

    class Args:
        sites, cells, lld, hoh, spin_mixing, no_positions, recur, workload, cells_given = 8, 10, 12, False, False, False, "block", "bcc", True
    W = bm.build_workload(Args(), 1)
    a_o, b_o = oracle.Oracle(dict(nn=W["nn"], iz=W["iz"], nmax=0, ee=W["ee"], lsham=W["lsham"], hoh=0, nsp=2)).block_lanczos(np.asarray(W["irec"], np.int32), 12)
    assert rel_err(a[..., 0] + 1j * a[..., 1], a_o) < RTOL and rel_err(b2[..., 0] + 1j * b2[..., 1], b_o) < RTOL
