"""libavc in more than one process: two rank processes (gloo, both on the box's one GPU) each
attack their contiguous shard through the HIP path and gather on the host -- bench.py's
multi-GPU data path with real kernels instead of the CPU stand-in of test_distributed.py.
The gathered result must equal one process attacking the whole batch bitwise (per-utterance
arithmetic never depends on the batch: DESIGN.md 5)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gpu_mp_worker as W  # noqa: E402

pytestmark = pytest.mark.gpu


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("kind,total", [("emb", 5), ("fb", 3)])
def test_two_rank_processes_match_single(tmp_path, kind, total):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    T, n, prec = 128, 6, "bf16"
    out = str(tmp_path / "full.npy")
    port = _port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "gpu_mp_worker.py"), kind, str(total),
                                       str(T), str(n), prec, out], env=env))
    codes = [p.wait(timeout=300) for p in procs]
    assert codes == [0, 0], codes
    got = np.load(out)
    vc, at, src, p0 = W.inputs(total, T)
    ref = W.run(kind, vc, at, src, p0, torch.device("cuda", 0), n, prec).detach().cpu().numpy()
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)


def test_bench_plain_run_dumps_its_outputs(tmp_path, monkeypatch, golden):
    """`bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR` in a fresh process: the line carries
    ms_per_step and no --full figure, and DIR/adv.npy is what attack_utils.emb_attack returns for the
    bench's seeded inputs (same kernels, same batch: bitwise)."""
    import json
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    B, T, n = 256, 128, 4           # the headline's shape (its tile choices are committed), a few iterations
    d = tmp_path / "dump"
    # bench.py's committed tile choices, as a copy: a shape missing from the file is tuned at first use and
    # appended to it, and the bench process and this one must launch the same kernels
    import shutil
    tune = str(tmp_path / "tune.txt")
    shutil.copyfile(os.path.join(os.path.dirname(HERE), "profiles", "tune_gfx950.txt"), tune)
    monkeypatch.setenv("AVC_TUNE_FILE", tune)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--batch", str(B), "--frames", str(T), "--n-iters", str(n),
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "utts/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert abs(line["value"] - B / (line["ms_per_step"] * 1e-3)) <= 1e-2 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["fp32"] is None
    assert sorted(os.listdir(d)) == ["adv.npy"]
    adv = np.load(d / "adv.npy")
    assert adv.dtype == np.float32 and adv.shape == (B, 80, T)
    import attack_utils
    from helpers import model_from_fixture
    dev = torch.device("cuda", 0)
    model = model_from_fixture(golden("full_T128")).to(dev)     # the full config, seed 0: bench.py's model
    g = torch.Generator().manual_seed(1)
    vc, at = torch.randn(B, 80, T, generator=g), torch.randn(B, 80, T, generator=g)
    p0 = torch.randn(B, 80, T, generator=torch.Generator().manual_seed(123))
    ref = attack_utils.emb_attack(model, vc.to(dev), at.to(dev), 0.1, n, ptb0=p0.to(dev), precision="bf16")
    assert np.array_equal(adv, ref.detach().cpu().numpy())
