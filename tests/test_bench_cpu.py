"""bench.py's rank launcher (no GPU needed): `--gpus N` with no launcher around it starts N
ranks under torch.distributed.run; a world that differs from --gpus is an error.  Also the
--dump-outputs writer on CPU tensors: names, dtype, the fixed sample positions."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(args, **env):
    e = {k: v for k, v in os.environ.items()
         if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e,
                          capture_output=True, text=True, timeout=120)


def test_launch_cmd_starts_n_ranks():
    import bench
    cmd = bench.launch_cmd(8, ["--gpus", "8", "--steps", "3"], 29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    i = cmd.index("--master-addr")
    assert cmd[i + 1] == "127.0.0.1" and "--master-port=29555" in cmd
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"]
    assert os.path.samefile(cmd[-5], os.path.join(ROOT, "bench.py"))


def test_world_mismatch_exits_nonzero():
    r = _run(["--gpus", "3", "--no-cpu-baseline"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2, r.stderr
    assert "--gpus 3 but the launcher started 2 ranks" in r.stderr


def test_too_few_gpus_for_rccl_exits_nonzero():
    import torch
    n = max(2, torch.cuda.device_count() + 1)
    r = _run(["--gpus", str(n), "--no-cpu-baseline"], MMDX_DIST_BACKEND="nccl")
    assert r.returncode == 2, r.stderr
    assert f"--gpus {n} needs {n} GPUs for RCCL" in r.stderr


def test_gpus_must_be_positive():
    r = _run(["--gpus", "0"])
    assert r.returncode != 0 and "--gpus must be >= 1" in r.stderr


def test_steps_must_be_positive():
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_dump_outputs_writes_float32_arrays_at_fixed_positions(tmp_path):
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(7)
    big = torch.randn(3 * bench.DUMP_SAMPLE + 5, generator=g, dtype=torch.float64)
    small = torch.randn(4, 3, generator=g).to(torch.bfloat16)
    nograd = torch.randn(6, generator=g)
    big.grad = big * 2
    small.grad = small + 1
    loss, logits = torch.tensor(0.625), torch.randn(5, 13, generator=g)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), loss, torch.tensor(1.5), logits,
                           [big, small, nograd])
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["grad_norm", "grads_sample", "logits", "loss", "params_sample"]
    assert all(v.dtype == np.float32 for v in got.values())
    for k, v in got.items():   # the same positions on every call
        assert np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy")))
    assert got["loss"].tolist() == [0.625] and got["grad_norm"].tolist() == [1.5]
    assert np.array_equal(got["logits"], logits.numpy())
    n = bench.DUMP_SAMPLE
    ps, gs = got["params_sample"], got["grads_sample"]
    assert ps.shape == gs.shape == (n + 12 + 6,)
    # the sampled positions are elements of the tensor, and the gradient is taken at the same ones
    assert np.isin(ps[:n], big.float().numpy()).all() and len(np.unique(ps[:n])) > n // 2
    assert np.array_equal(gs[:n], (ps[:n].astype(np.float64) * 2).astype(np.float32))
    assert np.array_equal(ps[n:n + 12], small.float().reshape(-1).numpy())
    assert np.array_equal(gs[n:n + 12], small.grad.float().reshape(-1).numpy())
    assert np.array_equal(ps[n + 12:], nograd.numpy()) and not gs[n + 12:].any()
