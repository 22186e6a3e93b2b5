"""GmmModel on the CPU: scoring the training data with a saved model gives
the training run's memberships exactly, chunking, save/load, .summary
parsing and the classify command line."""
import json
import os

import numpy as np
import pytest
import torch

from cuda_gmm_mpi_amd import GmmModel
from cuda_gmm_mpi_amd.classify import main as classify_main
from cuda_gmm_mpi_amd.cli import main as gmm_main, run_clustering
from cuda_gmm_mpi_amd.ops import cpu_reference as cpu
from cuda_gmm_mpi_amd.utils import io as gio
from cuda_gmm_mpi_amd.utils.config import GmmConfig
from cuda_gmm_mpi_amd.utils.synthetic import make_blobs

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "fixtures")
FIELDS = ("center", "means_centered", "pi", "N", "constant", "avgvar", "R",
          "Rinv")

# name -> config changes. "merged" runs no EM iteration, so the saved K=2
# model is what the bug_compat merge left: its constant carries the log10
# quirk and is not what compute_constants gives for its R.
CASES = {
    "full": dict(min_iters=5, max_iters=5),
    "diag": dict(min_iters=5, max_iters=5, diag_only=True),
    "merged": dict(min_iters=0, max_iters=0, bug_compat=True),
}


def first_argmax(w):
    return np.argmax(w, axis=0).astype(np.int32)  # numpy: first maximum


@pytest.fixture(scope="module")
def data():
    return make_blobs(2000, 3, 4, seed=7)[0]  # the small_blobs shape


@pytest.fixture(scope="module")
def trained(data, tmp_path_factory):
    """name -> (run_clustering result, model path, output stem)."""
    out = {}
    for name, extra in CASES.items():
        d = tmp_path_factory.mktemp(name)
        cfg = GmmConfig(num_clusters=4, target_num_clusters=2, **extra)
        path = str(d / "model.npz")
        stem = str(d / "train")
        out[name] = (run_clustering(data, cfg, stem, "cpu", save_model=path),
                     path, stem)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_scoring_training_data_reproduces_memberships(data, trained, name):
    result, path, _ = trained[name]
    assert result["num_clusters"] == 2
    model = GmmModel.load(path)
    assert model.diag_only == bool(CASES[name].get("diag_only", False))
    w = model.posteriors(data, device="cpu")
    assert w.dtype == np.float32 and w.shape == (2, 2000)
    assert np.array_equal(w, result["memberships"])
    pred = model.predict(data, device="cpu")
    assert pred.labels.dtype == np.int32
    assert np.array_equal(pred.labels, first_argmax(result["memberships"]))
    assert np.array_equal(pred.max_posterior, w.max(axis=0))
    assert pred.log_likelihood == float(pred.log_prob.astype(np.float64).sum())
    assert pred.counts.dtype == np.int64 and pred.counts.sum() == 2000
    assert np.array_equal(pred.counts, np.bincount(pred.labels, minlength=2))
    assert model.score(data, device="cpu") == pred.log_likelihood
    # the public means are the de-centred ones of the .summary state
    np.testing.assert_allclose(model.means.numpy(),
                               result["state"].means.numpy(), rtol=0,
                               atol=1e-5)


def test_merged_model_keeps_the_constant_verbatim(trained):
    """The case above proves nothing unless the saved constant really is
    the merge path's: it must differ from the natural-log recompute."""
    model = trained["merged"][0]["model"]
    _, recomputed = cpu.compute_constants(model.R)
    assert not np.allclose(model.constant.numpy(), recomputed.numpy(),
                           rtol=0, atol=1e-3)


def test_chunking(data, trained):
    model = trained["full"][0]["model"]
    one = model.predict(data, device="cpu")
    many = model.predict(data, device="cpu", chunk_events=7)
    assert np.array_equal(one.labels, many.labels)
    # CPU matmul blocking may differ with the batch size
    np.testing.assert_allclose(many.log_prob, one.log_prob, rtol=1e-5)
    np.testing.assert_allclose(many.max_posterior, one.max_posterior,
                               rtol=1e-5)
    np.testing.assert_allclose(
        model.posteriors(data, device="cpu", chunk_events=300),
        model.posteriors(data, device="cpu"), rtol=1e-5, atol=1e-30)


def test_save_load_round_trip(trained, tmp_path):
    model = trained["diag"][0]["model"]
    path = str(tmp_path / "m.npz")
    model.save(path)
    back = GmmModel.load(path)
    for name in FIELDS:
        a, b = getattr(model, name), getattr(back, name)
        assert b.dtype == torch.float32
        assert torch.equal(a, b), name
    assert back.diag_only is True and back.bug_compat is model.bug_compat
    assert torch.equal(back.means, back.means_centered + back.center)
    with np.load(path) as z:
        assert float(z["format_version"]) == 1.0
        assert all(z[k].dtype == np.float32 for k in z.files)
    assert os.listdir(tmp_path) == ["m.npz"]  # no temp file left


def test_bad_model_files(trained, tmp_path):
    good = trained["full"][1]
    blob = open(good, "rb").read()
    cut = str(tmp_path / "cut.npz")
    with open(cut, "wb") as f:
        f.write(blob[:len(blob) // 2])
    with pytest.raises(ValueError, match="cannot load model"):
        GmmModel.load(cut)
    with np.load(good) as z:
        fields = {k: z[k] for k in z.files}
    keys = str(tmp_path / "keys.npz")
    np.savez(keys, **{k: v for k, v in fields.items() if k != "Rinv"},
             extra=np.zeros(1, np.float32))
    with pytest.raises(ValueError, match="Rinv"):
        GmmModel.load(keys)
    shapes = str(tmp_path / "shapes.npz")
    np.savez(shapes, **dict(fields, pi=np.ones(3, np.float32)))
    with pytest.raises(ValueError, match="pi has shape"):
        GmmModel.load(shapes)


def test_summary_round_trip(trained, tmp_path):
    state = trained["full"][0]["state"]
    path = str(tmp_path / "s.summary")
    gio.write_summary(path, state)
    s = gio.read_summary(path)
    # %.3f holds means and R to half a unit of the third decimal, %f holds
    # pi and N to half a unit of the sixth
    np.testing.assert_allclose(s["means"], state.means.numpy(), rtol=0,
                               atol=5e-4)
    np.testing.assert_allclose(s["R"], state.R.numpy(), rtol=0, atol=5e-4)
    np.testing.assert_allclose(s["pi"], state.pi.numpy(), rtol=0, atol=5e-7)
    np.testing.assert_allclose(s["N"], state.N.numpy(), rtol=0, atol=5e-7)
    with pytest.raises(ValueError):
        gio.read_summary(trained["full"][1])  # a .npz is not a summary


def test_from_summary_fixture():
    path = os.path.join(FIXTURES, "golden_small.summary")
    k = open(path).read().count("Cluster #")
    data = gio.read_bin(os.path.join(FIXTURES, "golden_small.bin"))
    model = GmmModel.from_summary(path)
    assert model.num_clusters == k >= 1
    assert model.num_dimensions == data.shape[1]
    pred = model.predict(data, device="cpu")
    assert pred.labels.shape == (data.shape[0],)
    assert pred.labels.min() >= 0 and pred.labels.max() < k
    assert np.isfinite(pred.log_prob).all()
    assert np.all((pred.max_posterior >= 1.0 / k - 1e-6)
                  & (pred.max_posterior <= 1.0 + 1e-6))


def test_classify_cli(data, trained, tmp_path):
    _, model_path, stem = trained["full"]
    infile = str(tmp_path / "d.bin")
    gio.write_bin(infile, data)
    out = str(tmp_path / "scored")
    metrics = str(tmp_path / "m.json")
    rc = classify_main([model_path, infile, out, "--device", "cpu",
                        "--memberships", "--metrics-out", metrics,
                        "--chunk-events", "2000"])
    assert rc == 0
    lines = open(out + ".labels").read().splitlines()
    assert len(lines) == 2000
    pred = GmmModel.load(model_path).predict(data, device="cpu")
    for i in (0, 1, 999, 1999):
        assert lines[i] == "%d,%f,%f" % (pred.labels[i],
                                         pred.max_posterior[i],
                                         pred.log_prob[i])
    for ln in lines:
        lab, pm, lp = ln.split(",")
        assert lab in ("0", "1") and len(pm.split(".")[1]) == 6
        float(lp)
    # byte-equal to the .results the training run wrote for the same data
    assert (open(out + ".results", "rb").read()
            == open(stem + ".results", "rb").read())
    m = json.load(open(metrics))
    assert (m["N"], m["K"], m["D"], m["device"]) == (2000, 2, 3, "cpu")
    assert m["counts"] == pred.counts.tolist()
    assert m["log_likelihood"] == pred.log_likelihood
    assert m["seconds"] > 0


def test_classify_cli_exit_codes(data, trained, tmp_path, capsys):
    _, model_path, _ = trained["full"]
    infile = str(tmp_path / "d.bin")
    gio.write_bin(infile, data)
    out = str(tmp_path / "o")
    assert classify_main([model_path, str(tmp_path / "none.bin"), out,
                          "--device", "cpu"]) == 2
    assert classify_main([str(tmp_path / "none.npz"), infile, out,
                          "--device", "cpu"]) == 5
    assert classify_main([infile, infile, out, "--device", "cpu"]) == 5
    wide = str(tmp_path / "wide.bin")
    gio.write_bin(wide, np.zeros((10, 5), np.float32))
    capsys.readouterr()
    assert classify_main([model_path, wide, out, "--device", "cpu"]) == 5
    msg = capsys.readouterr().out.strip()
    assert "D=5" in msg and "D=3" in msg and "\n" not in msg
    assert not os.path.exists(out + ".labels")


def test_gmm_save_model_flag(data, tmp_path):
    infile = str(tmp_path / "d.bin")
    gio.write_bin(infile, data)
    out = str(tmp_path / "run")
    path = str(tmp_path / "run_model.npz")
    argv = ["4", infile, out, "2", "--min-iters", "3", "--max-iters", "3",
            "--device", "cpu"]
    assert gmm_main(argv) == 0
    assert not os.path.exists(path)  # off by default
    assert gmm_main(argv + ["--save-model", path]) == 0
    model = GmmModel.load(path)
    assert (model.num_clusters, model.num_dimensions) == (2, 3)
    summary = gio.read_summary(out + ".summary")
    np.testing.assert_allclose(model.means.numpy(), summary["means"],
                               rtol=0, atol=1e-3)
