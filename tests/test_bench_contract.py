"""bench.py honours the driver's contract: one JSON line with the agreed keys."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_small_workload():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                          "--warmup", "1", "--targets", "50000", "--cfg5-targets", "250000", "--cfg5-steps", "2", "--full"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["unit"] == "GCUPS" and line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1
    assert line["higher_is_better"] is True and line["scaling"] == "weak" and line["vs_baseline"] is None
    assert "workload" in line["config"] and "model" not in line["config"]
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-4 and roof["achieved"] > 0
    cpu = line["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] >= 1 and cpu["value"] > 0 and cpu["unit"] == "GCUPS"
    assert line["value"] > cpu["value"]
    # what the line says about itself: the host-visible form beside `value`, an honest CPU leg,
    # PMC-derived numbers only for the build they were measured on
    # `value` at N = 1 is the host-visible form (blocking call, scores in the caller's pinned host array);
    # the HBM-resident form and the pageable-array form stand beside it
    assert line["value_device_results"] and line["value"] <= line["value_device_results"] * 1.05
    # (at 50k targets a search takes 0.3 ms and the two host forms differ by less than their noise)
    assert line["value_host_results_pageable"] and line["value_host_results_pageable"] <= line["value"] * 1.3
    assert "pinned host array" in line["config"]["workload"] and line["forced_collective"] is False
    assert cpu["value_one_thread"] > 0 and cpu["cpu_model"] and cpu["host_physical_cores"] >= cpu["cores"] >= 1
    assert roof["traffic"] is None    # 50k targets is not the profiled workload
    # round 5: the printed line stays within 8 KB (a record that keeps its last 8 KB keeps all of it) and carries one
    # flat scalar per secondary leg inside `roofline`; everything nested is in bench_details.json beside it
    assert len(lines[0]) <= 8192, len(lines[0])
    assert all(not isinstance(v, (dict, list)) for v in roof.values()), roof
    # (valu_issue_frac / valu_instructions_per_cell_pair too when a PMC summary of this very build is committed)
    for key in ("pageable_gcups", "device_results_gcups", "pcie_inclusive_ms",
                "sustained_median_ms", "lognormal_gcups", "cfg2_end_ms", "q150_score_ms", "q150_end_ms", "q300_score_ms",
                "q300_end_ms", "cfg5_gcups"):
        assert roof.get(key) and roof[key] > 0, key
    assert "extras" not in line and line["details_file"] == "bench_details.json"
    with open(os.path.join(os.getcwd(), "bench_details.json")) as f:
        details = json.load(f)
    assert details["value"] == line["value"]
    assert "lds" in details["roofline"]
    assert set(details["roofline"]["valu_issue"]) >= {"achieved", "full_rate_peak", "frac", "cycles_per_instruction", "instructions_per_cell_pair"}
    strong = details["extras"]["cfg5_strong"]
    assert strong["scaling"] == "strong" and strong["gcups"] > 0 and sum(strong["targets_per_rank"]) == 250000
    assert strong["gcups"] == roof["cfg5_gcups"]
    assert "self_check" in strong
    # per-config rooflines of the secondary legs (the bound per config)
    for row in details["extras"]["longer_queries_sw"].values():
        for leg in row.values():
            assert leg["roofline"]["bound"] == "hbm" and leg["roofline"]["kernel_ms"] > 0 and leg["roofline"]["frac"] > 0


@pytest.mark.gpu
def test_bench_forced_collective_on_one_gpu():
    # the N > 1 path on the one GPU there is: a 1-rank nccl group under torch.distributed.run, RCCL's gather
    # of device tensors behind the search (stream ordering, MIOPAL_RESERVE_CUS), all_reduce of the elapsed
    # time, the self-check of the sharded cfg5 leg
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--targets", "50000", "--cfg5-targets", "250000", "--cfg5-steps", "2", "--force-collective", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["forced_collective"] is True and line["n_gpus"] == 1 and line["value"] > 0
    assert "RCCL gather" in line["config"]["workload"]
    assert line["roofline"]["cfg5_gcups"] > 0


@pytest.mark.gpu
def test_bench_starts_its_own_ranks():
    # `python bench.py --gpus 2` typed bare, as the driver types it: the parent spawns torch.distributed.run
    # itself (before anything touches the GPU) and relays rank 0's line. Rehearsal switches for a box with one
    # GPU: both ranks on cuda:0, gather through gloo. The line is complete at N > 1: roofline, cpu_baseline,
    # the self-checking cfg5 leg.
    env = dict(os.environ, MIOPAL_BENCH_SHARE_DEVICE="1", MIOPAL_BENCH_BACKEND="gloo")
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(key, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                          "--targets", "50000", "--cfg5-targets", "250000", "--cfg5-steps", "2", "--full"],
                         capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["value"] > 0 and line["scaling"] == "weak"
    assert line["roofline"]["kernel_ms"] > 0 and line["roofline"]["bound"] == "hbm"
    cpu = line["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1
    assert len(lines[0]) <= 8192 and line["roofline"]["cfg5_gcups"] > 0
    with open(os.path.join(os.getcwd(), "bench_details.json")) as f:
        strong = json.load(f)["extras"]["cfg5_strong"]
    assert "self_check" in strong and len(strong["targets_per_rank"]) == 2 and sum(strong["targets_per_rank"]) == 250000
    assert "RCCL gather" in line["config"]["workload"]


def test_bench_parent_spawns_before_touching_torch(tmp_path):
    # CPU tier: with --gpus 2 and no WORLD_SIZE the parent must hand over to torch.distributed.run WITHOUT
    # importing torch (a process that has initialised the GPU must not start the ranks). A stand-in
    # interpreter records what it was asked to run; the ranks themselves need GPUs (the GPU tier runs them).
    probe = tmp_path / "probe.py"
    probe.write_text(
        "import sys, json, runpy\n"
        "import bench\n"
        "seen = {}\n"
        "class P:\n"
        "    def __init__(self, cmd, **kw):\n"
        "        seen['cmd'] = cmd; seen['torch'] = 'torch' in sys.modules; self.stdout = iter(['{\"ok\": 1}\\n'])\n"
        "    def wait(self): return 7\n"
        "import subprocess; subprocess.Popen = P\n"
        "sys.argv = ['bench.py', '--gpus', '2', '--steps', '3']\n"
        "try:\n"
        "    bench.main()\n"
        "except SystemExit as e:\n"
        "    seen['code'] = e.code\n"
        "print(json.dumps(seen))\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(key, None)
    out = subprocess.run([sys.executable, str(probe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[0] == '{"ok": 1}'                      # the child's line is relayed
    seen = json.loads(lines[-1])
    assert seen["code"] == 7 and seen["torch"] is False
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=2" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "2", "--steps", "3"]


def test_bench_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0",
                          "--targets", "100"], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "needs a GPU" in (out.stderr + out.stdout)


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    # without --full: the headline figure alone (no secondary leg, no CPU baseline, no bench_details.json) and, with
    # --dump-outputs, the scores of the last timed step - the same on every run, equal to the CPU checker
    import numpy as np
    import _data
    import _oracle
    from pyopal_amd.matrices import ScoringMatrix
    n = 50000
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                          "--targets", str(n), "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 4 and line["warmup"] == 1 and line["unit"] == "GCUPS" and line["dtype"] == "u16"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] - 53.0 * n * 300 / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.002 * line["value"] + 0.1
    assert line["roofline"]["kernel_ms"] > 0
    for key in ("cpu_baseline", "extras", "details_file", "value_device_results", "value_pcie_inclusive"):
        assert key not in line, key
    assert not (tmp_path / "bench_details.json").exists()
    scores = np.load(tmp_path / "dump" / "scores.npy")
    assert scores.dtype == np.float32 and scores.shape == (n,)
    assert int(scores.astype(np.int64).sum()) == line["score_checksum"]
    # the inputs are those of the command line alone: seed 1, the README query
    residues, offsets = _data.random_db(np.random.default_rng(1), np.full(n, 300))
    matrix = np.array(ScoringMatrix.from_name("BLOSUM62").int_array(), dtype=np.int32)
    want = _oracle.search(_oracle.encode(_data.README_QUERY), residues[:offsets[512]], offsets[:513], matrix, 3, 1,
                          "score", "sw")["score"]
    assert np.array_equal(scores[:512], want.astype(np.float32))


def test_bench_dump_of_a_large_output_is_a_fixed_sample(tmp_path):
    import numpy as np
    import bench
    scores = np.arange(bench.DUMP_VALUES + 12345, dtype=np.int32)
    for where in ("a", "b"):
        bench.dump_outputs(str(tmp_path / where), scores)
    a, b = np.load(tmp_path / "a" / "scores.npy"), np.load(tmp_path / "b" / "scores.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_VALUES,) and a.nbytes <= 64 << 20
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)
    small = np.array([3, 0, 583], dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "c"), small)
    assert np.load(tmp_path / "c" / "scores.npy").tolist() == [3.0, 0.0, 583.0]
