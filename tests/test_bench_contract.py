"""bench.py's host-side contract (no GPU): defaults, how `--gpus N` starts its own ranks, what --dump-outputs writes, and
that the committed PMC profile still names the kernel the roofline object quotes (a tile-config change without a re-profile
would leave `roofline.traffic` null).  One GPU test: a plain run prints the headline line only and dumps its last step."""
import csv
import json
import os
import subprocess
import sys
import types
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_defaults_are_one_gpu_and_a_run_of_minutes():
    a = bench.parse_args([])
    assert a.gpus == 1 and 1 <= a.warmup <= 10 and 10 <= a.steps <= 100
    assert not (a.no_cpu_baseline or a.no_vfeat or a.no_e2e)
    assert not a.full and a.dump_outputs is None                    # a plain run: the headline only, nothing written


def test_gpus_n_without_a_launcher_spawns_torch_distributed_run(monkeypatch):
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return R()
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    argv = ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    rc = bench.spawn_ranks(bench.parse_args(argv), argv)
    cmd = seen["cmd"]
    assert rc == 7                                                   # the children's exit code is the parent's
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    assert cmd[-len(argv) - 1] == os.path.join(ROOT, "bench.py") and cmd[-len(argv):] == argv
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_committed_pmc_profile_names_the_roofline_kernel():
    nbytes, src = bench.pmc_traffic()
    assert src == "profiles/" + bench.PMC_TRAFFIC_FILES[0], "the newest committed profile must name the roofline kernel"
    # between the algorithmic minimum (235 MB) and an order of magnitude above it
    assert 235e6 <= nbytes <= 2.5e9
    # the same kernel, with the same grid, is in the committed kernel trace
    want = bench.ROOFLINE_KERNEL.split(" (")[0].replace(" ", "")
    with open(os.path.join(ROOT, "profiles", "r4_kernel_stats.csv")) as f:
        names = [r["Name"].replace(" ", "") for r in csv.DictReader(f)]
    assert any(want in n for n in names), want


def test_flops_and_peak_constants():
    # 2 * (512*36) * 1024 * 2048 FLOP per launch of the roofline GEMM; f32-input MFMA peak of the guide
    assert bench.F32_MFMA_PEAK_TFLOPS == pytest.approx(157.3)
    cfg = bench.CFG
    assert (cfg["B"], cfg["R"], cfg["D"], cfg["H"], cfg["T"], cfg["A"]) == (512, 36, 2048, 1024, 14, 3000)


def test_tools_and_entry_points_compile():
    """every script under tools/ (some are driven by tests and by the profile recipes) and the two root entry points
    are at least syntactically valid python"""
    import glob
    paths = sorted(glob.glob(os.path.join(ROOT, "tools", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "dbg", "*.py")))
    paths += [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    assert len(paths) > 15
    for p in paths:
        with open(p) as f:
            compile(f.read(), p, "exec")


class _FakeEngine:
    """the part of FusionEngine that bench.dump_outputs reads, on the CPU"""

    def __init__(self, B, A, seed):
        import torch
        g = torch.Generator().manual_seed(seed)
        self.dims = types.SimpleNamespace(B=B, A=A)
        self.train_names = ["big/kernel", "small/bias"]
        self.params = {"big/kernel": torch.randn(20, 30, generator=g), "small/bias": torch.randn(5, generator=g)}
        self.grads = {k: 2 * v for k, v in self.params.items()}
        logit = torch.randn(B * A, generator=g)
        self._t = {"report": torch.arange(16, dtype=torch.float32), "logit": logit,
                   "pred": logit.view(B, A).argmax(1).to(torch.int32)}

    def check_recurrence(self):
        pass

    def tensor(self, name):
        return self._t[name]


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_of_large_variables(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    B, A = 4, 10
    eng = _FakeEngine(B, A, seed=0)
    total = bench.dump_outputs(eng, str(tmp_path / "a"))
    bench.dump_outputs(_FakeEngine(B, A, seed=0), str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["report.npy", "logit.npy", "pred.npy", "param.big.kernel.npy", "grad.big.kernel.npy",
                            "param.small.bias.npy", "grad.small.bias.npy"])
    d = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert sum(a.nbytes for a in d.values()) == total
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert d["report"].dtype == np.float64 and np.array_equal(d["report"], np.arange(13))
    assert d["logit"].shape == (B, A) and np.array_equal(d["pred"], d["logit"].argmax(1))
    # a variable of more than DUMP_SAMPLE elements: that many positions, ascending, seeded by the variable's name
    big = eng.params["big/kernel"].numpy().reshape(-1)
    pos = np.sort(np.random.default_rng(zlib.crc32(b"big/kernel")).choice(big.size, 64, replace=False))
    assert np.array_equal(d["param.big.kernel"], big[pos]) and np.array_equal(d["grad.big.kernel"], 2 * big[pos])
    assert np.array_equal(d["param.small.bias"], eng.params["small/bias"].numpy())
    for n in names:                                                  # the same inputs give the same files
        assert np.array_equal(d[n[:-4]], np.load(tmp_path / "b" / n))


def test_synthetic_batches_are_seeded_and_repeat_no_token():
    """one addend per embedding row in the scatter-add of its gradient: no summation order for the float atomics"""
    import torch
    cfg = dict(bench.CFG, B=64, T=14, A=50, Vq=2000)
    a = bench.synth_batches(cfg, torch.Generator().manual_seed(3), "cpu", 3)
    b = bench.synth_batches(cfg, torch.Generator().manual_seed(3), "cpu", 3)
    for x, y in zip(a, b):
        q = x["q_intseq"]
        assert q.dtype == torch.int32 and tuple(q.shape) == (64, 14) and q.is_contiguous()
        assert q.unique().numel() == q.numel() and 0 <= int(q.min()) and int(q.max()) < cfg["Vq"] - 3
        assert all(torch.equal(x[k], y[k]) for k in x)


def _plain_run(out, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    import numpy as np
    out = tmp_path / "dump"
    d = _plain_run(out, steps=3, warmup=1)
    assert d["metric"] == "VQA train samples/sec (img+question) at bs512" and d["unit"] == "samples/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(512 * 1e3 / d["ms_per_step"], rel=1e-6)
    assert not set(d) & {"cpu_baseline", "vfeat", "e2e", "pretrain", "experiment_bf16x3"}
    assert d["roofline"]["groups"] is None and d["roofline"]["clock"] is None
    a = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in a.values())
    assert a["report"][0] == pytest.approx(d["final_train_loss"], rel=1e-6)
    assert a["logit"].shape == (512, 3000) and np.array_equal(a["pred"], a["logit"].argmax(1))
    assert len([n for n in a if n.startswith("param.")]) == len([n for n in a if n.startswith("grad.")]) == 15


@pytest.mark.gpu
def test_two_runs_dump_the_same_bits(tmp_path):
    """same arguments, same inputs, same computation: after several steps of training both runs' outputs are identical"""
    import numpy as np
    da = _plain_run(tmp_path / "a", steps=4, warmup=2)
    db = _plain_run(tmp_path / "b", steps=4, warmup=2)
    assert da["final_train_loss"] == db["final_train_loss"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)), n
