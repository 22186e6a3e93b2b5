"""The classify kernels (estep_classify / estep_classify_f32) and
GmmModel.predict on the GPU.

The kernels copy the log-weight and log-sum-exp arithmetic of the training
kernels estep_fused / estep_fused_f32, so lse is compared bit for bit: with
the committed family fixtures and with a run of the training kernels on the
same staged z. The label is the first argmax of their log-weights.

pmax tolerance: pmax is compared with exp(max(w) - lse) in float64 at
atol = 1e-5. The assigned posterior is at least 1/K, so |m - lse| <=
ln 512 ~= 6.2; __expf is a scaled v_exp_f32 with a relative error of about
(1 + 6.2 * 1.44) * 2^-24 ~= 6e-7 on a value <= 1: more than a tenfold
margin."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd import GmmModel  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(9, 24, 313), (5, 31, 257), (3, 1, 300)]
PMAX_ATOL = 1e-5
# the project's bands for the fused kernels against the CPU ops
# (test_estep_fused_matches_cpu; the f32 lds test)
BANDS = {"bf16": dict(rtol=5e-2, atol=2e-2), "fp32": dict(rtol=2e-3, atol=2e-4)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def from_bits(a, device):
    """uint16 bit patterns -> bf16 tensor."""
    return torch.from_numpy(a.view(np.int16)).to(device).view(torch.bfloat16)


def load_fixture(dtype, k, d, n, device):
    """(x event-major fp32 [n, d], factor table, add, w, lse) of a family
    fixture of the training kernel of `dtype`."""
    stem = "estep_fused" if dtype == "bf16" else "estep_fused_f32"
    g = np.load(os.path.join(GOLDEN, f"{stem}_k{k}_d{d}_n{n}.npz"))
    if dtype == "bf16":
        x = from_bits(g["z"], device).float().T.contiguous()
        fac = from_bits(g["mfac"], device)
    else:
        x = torch.from_numpy(g["x"]).to(device).T.contiguous()
        fac = torch.from_numpy(g["mfac32"]).to(device)
    add = torch.from_numpy(g["add"]).to(device)
    assert x.shape == (n, d) and add.shape == (k,)
    return x, fac, add, g["w"], g["lse"]


def run_classify(dtype, x, center, fac, add):
    """Launch into pre-filled outputs; returns numpy (label, lse, pmax)."""
    n = x.shape[0]
    label = torch.full((n,), -1, dtype=torch.int32, device=x.device)
    lse = torch.full((n,), float("nan"), dtype=torch.float32, device=x.device)
    pmax = torch.full_like(lse, float("nan"))
    entry = "estep_classify" if dtype == "bf16" else "estep_classify_f32"
    getattr(hip_ext(), entry)(x, center, fac, add, label, lse, pmax)
    return label.cpu().numpy(), lse.cpu().numpy(), pmax.cpu().numpy()


def check_against_logw(got, w, lse):
    """got = (label, lse, pmax) against log-weights w [K, n] and their lse."""
    label, lse_c, pmax = got
    assert np.array_equal(lse_c, lse), "lse differs from the training kernel"
    assert np.array_equal(label, np.argmax(w, axis=0)), "label != first argmax"
    want = np.exp(w.max(axis=0).astype(np.float64) - lse.astype(np.float64))
    np.testing.assert_allclose(pmax, want, rtol=0, atol=PMAX_ATOL)


@pytest.mark.parametrize("k,d,n", SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_golden(dev, dtype, k, d, n):
    x, fac, add, w, lse = load_fixture(dtype, k, d, n, dev)
    center = torch.zeros(d, dtype=torch.float32, device=dev)
    got = run_classify(dtype, x, center, fac, add)
    check_against_logw(got, w, lse)
    if k == 9:  # clusters owned by all four waves win somewhere
        assert set(np.unique(got[0]) % 4) == {0, 1, 2, 3}


# K below the wave count; a partial block; full tile only; the K=9 shape;
# K above the lds bound with three blocks and a tail of one event
DIFF_SHAPES = [(1, 5, 64), (6, 2, 255), (17, 16, 256), (9, 24, 313),
               (130, 31, 513)]


def random_model(rng, k, d, device):
    means = torch.from_numpy(
        rng.standard_normal((k, d)).astype(np.float32) * 2).to(device)
    rs = []
    for _ in range(k):
        a = rng.standard_normal((d, d))
        rs.append((a @ a.T + d * np.eye(d)).astype(np.float32))
    r = torch.from_numpy(np.stack(rs)).to(device)
    pi = torch.from_numpy(
        rng.dirichlet(np.ones(k)).astype(np.float32)).to(device)
    return means, r, pi


@pytest.mark.parametrize("k,d,n", DIFF_SHAPES)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_matches_training_kernel(dev, dtype, k, d, n):
    """Non-zero centre: both sides stage the same fp32 x - center."""
    rng = np.random.default_rng(1000 * k + d)
    means, r, pi = random_model(rng, k, d, dev)
    mfac = torch.empty(k, 2, 32, 32, dtype=torch.bfloat16, device=dev)
    mfac32 = (torch.empty(k, 32, 32, dtype=torch.float32, device=dev)
              if dtype == "fp32" else None)
    _, const = F.constants(r, means, False, mfac, mfac32)
    add = const + torch.log(pi)
    fac = mfac32 if dtype == "fp32" else mfac
    center = torch.from_numpy(
        rng.standard_normal(d).astype(np.float32) * 3).to(dev)
    x = (torch.from_numpy(
        rng.standard_normal((n, d)).astype(np.float32) * 2).to(dev)
        + center.unsqueeze(0))
    z = (x - center.unsqueeze(0)).T.contiguous()
    w_out = torch.empty(k, n, dtype=torch.float32, device=dev)
    lse = torch.empty(n, dtype=torch.float32, device=dev)
    if dtype == "bf16":
        F.estep_fused(z.to(torch.bfloat16), fac, add, w_out, lse,
                      need_lik=False)
    else:
        F.estep_fused_f32(z, fac, add, w_out, lse, need_lik=False)
    got = run_classify(dtype, x, center, fac, add)
    check_against_logw(got, w_out.cpu().numpy(), lse.cpu().numpy())
    # the public wrapper returns the same arrays
    lab, ls, pm = F.estep_classify(x, center, fac, add, dtype)
    assert np.array_equal(lab.cpu().numpy(), got[0])
    assert np.array_equal(ls.cpu().numpy(), got[1])
    assert np.array_equal(pm.cpu().numpy(), got[2])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("shape,keep", [((3, 1, 300), 3), ((9, 24, 313), 4)])
def test_ties_go_to_the_lowest_cluster(dev, dtype, shape, keep):
    """The first `keep` clusters twice: K=3 doubled puts c and c+3 in
    different waves, four clusters doubled put c and c+4 in the same wave."""
    k, d, n = shape
    x, fac, add, w, _ = load_fixture(dtype, k, d, n, dev)
    fac2 = torch.cat([fac[:keep], fac[:keep]]).contiguous()
    add2 = torch.cat([add[:keep], add[:keep]]).contiguous()
    center = torch.zeros(d, dtype=torch.float32, device=dev)
    label, lse, pmax = run_classify(dtype, x, center, fac2, add2)
    assert label.max() < keep
    assert np.array_equal(label, np.argmax(w[:keep], axis=0))
    assert np.isfinite(lse).all() and np.all(pmax <= 0.5 + PMAX_ATOL)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The CPU tests' model: small_blobs shape, K = 4 -> 2, on the CPU."""
    from cuda_gmm_mpi_amd.cli import run_clustering
    from cuda_gmm_mpi_amd.utils.config import GmmConfig
    from cuda_gmm_mpi_amd.utils.synthetic import make_blobs
    data = make_blobs(2000, 3, 4, seed=7)[0]
    cfg = GmmConfig(num_clusters=4, target_num_clusters=2, min_iters=5,
                    max_iters=5)
    stem = str(tmp_path_factory.mktemp("train") / "train")
    result = run_clustering(data, cfg, stem, "cpu", write_results=False)
    return data, result["model"]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_predict_chunk_independent(trained, dtype):
    data, model = trained
    data = data[:1000]
    one = model.predict(data, device="cuda", estep_dtype=dtype)
    many = model.predict(data, device="cuda", estep_dtype=dtype,
                         chunk_events=300)
    assert np.array_equal(one.labels, many.labels)
    assert np.array_equal(one.log_prob, many.log_prob)
    assert np.array_equal(one.max_posterior, many.max_posterior)
    assert one.log_likelihood == many.log_likelihood


def check_against_cpu(model, data, dtype):
    band = BANDS[dtype]
    ref = model.predict(data, device="cpu")
    got = model.predict(data, device="cuda", estep_dtype=dtype)
    np.testing.assert_allclose(got.log_prob, ref.log_prob, **band)
    np.testing.assert_allclose(got.max_posterior, ref.max_posterior, **band)
    w = np.sort(model.posteriors(data, device="cpu"), axis=0)
    clear = (w[-1] - w[-2]) > band["atol"] if w.shape[0] > 1 else w[-1] > 0
    share = 1.0 - clear.mean()
    print(f"{dtype}: {100 * share:.3f} % of events within {band['atol']} "
          "of a tie on the CPU")
    assert share <= 0.02
    assert np.array_equal(got.labels[clear], ref.labels[clear])
    assert got.counts.sum() == data.shape[0]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_predict_matches_cpu(trained, dtype):
    data, model = trained
    check_against_cpu(model, data, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_predict_big_d_fallback(dtype):
    """D > 31 goes through the log-weight kernels per chunk."""
    rng = np.random.default_rng(40)
    k, d, n = 3, 40, 500
    means, r, pi = random_model(rng, k, d, "cpu")
    means = means * 3
    model = GmmModel.from_params(means, r, pi)
    which = rng.integers(0, k, n)
    chol = torch.linalg.cholesky(r.double())
    noise = torch.from_numpy(rng.standard_normal((n, d)))
    data = (means[which].double()
            + torch.einsum("nij,nj->ni", chol[which], noise)).float().numpy()
    assert not F.estep_classify_available(torch.device("cuda"), d)
    check_against_cpu(model, data, dtype)


def test_argument_checks(dev):
    k, d, n = 3, 4, 100
    x = torch.zeros(n, d, device=dev)
    center = torch.zeros(d, device=dev)
    fac = torch.zeros(k, 32, 32, device=dev)
    facb = torch.zeros(k, 2, 32, 32, dtype=torch.bfloat16, device=dev)
    add = torch.zeros(k, device=dev)

    def outs(m=n, ldt=torch.int32):
        return (torch.zeros(m, dtype=ldt, device=dev),
                torch.zeros(m, device=dev), torch.zeros(m, device=dev))
    ext = hip_ext()
    ext.estep_classify_f32(x, center, fac, add, *outs())  # the valid call
    ext.estep_classify(x, center, facb, add, *outs())
    with pytest.raises(RuntimeError):  # wrong dtype: x
        ext.estep_classify_f32(x.double(), center, fac, add, *outs())
    with pytest.raises(RuntimeError):  # wrong dtype: table
        ext.estep_classify(x, center, fac, add, *outs())
    with pytest.raises(RuntimeError):  # wrong dtype: label
        ext.estep_classify_f32(x, center, fac, add, *outs(ldt=torch.int64))
    with pytest.raises(RuntimeError):  # D = 32
        ext.estep_classify_f32(torch.zeros(n, 32, device=dev),
                               torch.zeros(32, device=dev), fac, add, *outs())
    with pytest.raises(RuntimeError):  # non-contiguous x
        ext.estep_classify_f32(torch.zeros(d, n, device=dev).T, center, fac,
                               add, *outs())
    with pytest.raises(RuntimeError):  # short output
        ext.estep_classify_f32(x, center, fac, add, *outs(n - 1))
    with pytest.raises(RuntimeError):  # table too small for K
        ext.estep_classify_f32(x, center, fac[:2], add, *outs())
    with pytest.raises(RuntimeError):  # centre of another D
        ext.estep_classify_f32(x, center[:3].contiguous(), fac, add, *outs())
