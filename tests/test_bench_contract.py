"""The driver depends on bench.py's exact CLI + one-line JSON contract."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    if env_extra:
        env.update(env_extra)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py")] + args,
        capture_output=True, text=True, timeout=timeout, env=env, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE json line, got: {out.stdout!r}"
    return json.loads(lines[0])


def check_contract(d, n_gpus):
    assert d["metric"] == "em_iterations_per_sec"
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["n_gpus"] == n_gpus
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-6
    assert d["data"] == "synthetic"
    assert d["config"]["parallelism"] == f"dp{n_gpus}"
    for key in ("steps", "warmup", "dtype", "vs_baseline"):
        assert key in d


@pytest.mark.timeout(600)
def test_bench_single_process_cpu():
    d = run_bench(["--steps", "2", "--warmup", "1",
                   "--events-per-gpu", "3000"])
    check_contract(d, 1)
    assert d["config"]["n_events"] == 3000


@pytest.mark.timeout(600)
def test_bench_full_and_dump_outputs_cpu(tmp_path):
    """--full keeps the one-line contract, and --dump-outputs writes the
    last step's outputs as small float .npy files that repeat from run
    to run (same arguments -> same inputs -> same outputs)."""
    import numpy as np
    args = ["--steps", "2", "--warmup", "1", "--events-per-gpu", "3000",
            "--clusters", "5", "--dims", "4"]
    dumps = []
    for name, extra in (("a", ["--full"]), ("b", [])):
        out_dir = tmp_path / name
        d = run_bench(args + extra + ["--dump-outputs", str(out_dir)])
        check_contract(d, 1)
        assert d["steps"] == 2 and d["dtype"] in d["modes"]
        dumps.append({p.stem: np.load(p) for p in out_dir.glob("*.npy")})
    a, b = dumps
    assert set(a) == set(b) == {"N", "pi", "means", "R", "constant",
                                "likelihood", "posteriors_sample"}
    assert a["means"].shape == (5, 4) and a["R"].shape == (5, 4, 4)
    assert a["posteriors_sample"].shape == (5, 3000)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.all(np.isfinite(a[name])), name
        np.testing.assert_allclose(a[name], b[name], rtol=1e-5, atol=1e-6,
                                   err_msg=name)
    np.testing.assert_allclose(a["posteriors_sample"].sum(axis=0), 1.0,
                               atol=1e-4)
    np.testing.assert_allclose(a["N"].sum(), 3000.0, rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_full_and_dump_outputs_gpu(tmp_path):
    """On the GPU --full adds the other precision to `modes`; the dump
    holds the headline (bf16) mode's last step, posteriors sampled."""
    import numpy as np
    d = run_bench(["--gpus", "1", "--steps", "3", "--warmup", "2",
                   "--events-per-gpu", "100000", "--full",
                   "--dump-outputs", str(tmp_path)], timeout=280)
    check_contract(d, 1)
    assert d["dtype"] == "bf16" and set(d["modes"]) == {"bf16", "fp32"}
    assert d["modes"]["bf16"]["ms_per_step"] == d["ms_per_step"]
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(got) == {"N", "pi", "means", "R", "constant", "likelihood",
                        "posteriors_sample"}
    assert got["R"].shape == (64, 24, 24)
    assert got["posteriors_sample"].shape == (64, 32768)
    for name, a in got.items():
        assert a.dtype == np.float32 and np.all(np.isfinite(a)), name
    np.testing.assert_allclose(got["posteriors_sample"].sum(axis=0), 1.0,
                               atol=1e-3)
    np.testing.assert_allclose(got["pi"].sum(), 1.0, atol=1e-3)


@pytest.mark.timeout(900)
def test_bench_torchrun_world2_cpu():
    """The driver's exact launch form, world 2 on gloo."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    # a CPU test wherever it runs: on a one-GPU box both ranks would
    # otherwise land on that GPU and RCCL refuses ("Duplicate GPU")
    env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = "-1"
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29733", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1", "--events-per-gpu", "2000"],
        capture_output=True, text=True, timeout=600, env=env, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    check_contract(d, 2)
    assert d["config"]["n_events"] == 4000  # weak scaling: 2000/rank
