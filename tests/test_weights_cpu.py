"""Per-event training weights on the CPU engine path: a weight s_e makes
event e count as s_e observations, 0 leaves it out of the fit.

Tolerances are not picked: the reordering floor below is measured on the
unweighted engine alone (the same fit on the same rows in two row orders),
and the weighted comparisons allow 8x that. Differences are relative to the
scale of the compared quantity, max|a - b| / max|b|, so one number serves
N, pi, means, R and the likelihood.
"""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from cuda_gmm_mpi_amd.engine import EmEngine, build_engine
from cuda_gmm_mpi_amd.ops import cpu_reference as cpu
from cuda_gmm_mpi_amd.utils.config import GmmConfig
from cuda_gmm_mpi_amd.utils.synthetic import make_supported_blobs

D, K, N_BASE, ITERS = 3, 3, 600, 5

# Reordering noise floor of the unweighted CPU engine at this shape: the
# largest scale-relative difference over N, pi, means, R and the likelihood
# between the replicated rows and a fixed permutation of them. Measured:
# 8.6e-6, carried by R (the fp32 cancellation in S - N mu mu^T; means move
# by 2e-8, the likelihood by at most 8e-8, N and pi not at all: the blobs
# are separated well enough for 0/1 posteriors). The `replicated` fixture
# re-measures it on every run (it is a property of the fp32 sums of the
# machine's BLAS) and the tests allow FLOOR_FACTOR times what it measures:
# the weighted run changes both the grouping and the order of the sums, and
# a single permutation samples only one reordering.
REORDER_FLOOR_MEASURED = 8.6e-6
FLOOR_FACTOR = 8.0

KEYS = ("N", "pi", "means", "R", "lik")


def cfg_for(k=K, iters=ITERS, **kw):
    return GmmConfig(num_clusters=k, target_num_clusters=k,
                     min_iters=iters, max_iters=iters, **kw)


def collect(eng, k=K):
    lik = eng.run_em(k)
    st = eng.state.shrink(k)
    return {"N": st.N.numpy().astype(np.float64),
            "pi": st.pi.numpy().astype(np.float64),
            # file-frame means: two engines may centre differently
            "means": (st.means + eng.center.unsqueeze(0)).numpy()
            .astype(np.float64),
            "R": st.R.numpy().astype(np.float64),
            "lik": np.array([lik], dtype=np.float64)}


def reldiff(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def worst(a, b, keys=KEYS):
    return max(reldiff(a[q], b[q]) for q in keys)


@pytest.fixture(scope="module")
def base():
    data, labels = make_supported_blobs(N_BASE, D, K, seed=11)
    s = np.random.default_rng(5).integers(0, 4, size=N_BASE)
    return data, labels, s.astype(np.float32)


def direct_engine(rows, total, center, seeds, var, weights=None):
    return EmEngine(torch.from_numpy(rows), cfg_for(), total, center, seeds,
                    var, device="cpu",
                    weights_shard=(None if weights is None
                                   else torch.from_numpy(weights)))


@pytest.fixture(scope="module")
def replicated(base):
    """Replicated rows, the shared seeding inputs, the unweighted reference
    fit on them and the measured reordering floor (parent code only)."""
    data, labels, s = base
    rows = np.repeat(data, s.astype(np.int64), axis=0)
    total = int(s.sum())
    assert rows.shape[0] == total
    rt = torch.from_numpy(rows).double()
    center = rt.mean(dim=0).float()
    var = (rt.pow(2).mean(dim=0) - rt.mean(dim=0).pow(2)).float()
    # one seed per blob, from events that carry weight
    seeds = torch.from_numpy(np.stack([
        data[np.nonzero((labels == c) & (s > 0))[0][0]] for c in range(K)]))
    ref = collect(direct_engine(rows, total, center, seeds, var))
    perm = np.random.default_rng(99).permutation(total)
    ref_p = collect(direct_engine(np.ascontiguousarray(rows[perm]), total,
                                  center, seeds, var))
    floor = worst(ref_p, ref)
    print(f"reordering floor: {floor:.3e}")
    assert floor > 0.0
    return {"rows": rows, "total": total, "center": center, "var": var,
            "seeds": seeds, "ref": ref, "floor": floor}


def test_integer_weights_equal_replicated_rows(base, replicated):
    data, _, s = base
    r = replicated
    eng = direct_engine(data, r["total"], r["center"], r["seeds"], r["var"],
                        weights=s)
    assert eng.n_total == r["total"]
    got = collect(eng)
    for q in KEYS:
        diff = reldiff(got[q], r["ref"][q])
        print(f"{q}: {diff:.3e} (floor {r['floor']:.3e})")
    assert worst(got, r["ref"]) <= FLOOR_FACTOR * r["floor"]


def test_mask_equals_subset(base, replicated, monkeypatch):
    import cuda_gmm_mpi_amd.engine as engine_mod
    data, _, s = base
    mask = (s > 0).astype(np.float32)
    seeds = []
    orig = engine_mod.seed_means_host

    def spy(rows, k):
        seeds.append(orig(rows, k))
        return seeds[-1]

    monkeypatch.setattr(engine_mod, "seed_means_host", spy)
    eng_w = build_engine(data, cfg_for(), device="cpu", weights=mask)
    eng_s = build_engine(data[mask > 0], cfg_for(), device="cpu")
    # strided seeds are drawn from the kept events in file order: bitwise
    # the subset's seeds
    assert torch.equal(seeds[0], seeds[1])
    assert eng_w.n_total == eng_s.n_total == int(mask.sum())
    assert torch.equal(eng_w.state.N, eng_s.state.N)
    got, ref = collect(eng_w), collect(eng_s)
    for q in KEYS:
        print(f"{q}: {reldiff(got[q], ref[q]):.3e}")
    assert worst(got, ref) <= FLOOR_FACTOR * replicated["floor"]


def test_all_ones_equal_unweighted(base, replicated):
    data = base[0]
    eng_w = build_engine(data, cfg_for(), device="cpu",
                         weights=np.ones(N_BASE, np.float32))
    eng_u = build_engine(data, cfg_for(), device="cpu")
    assert eng_w.n_total == eng_u.n_total
    assert eng_w.epsilon == eng_u.epsilon
    got, ref = collect(eng_w), collect(eng_u)
    assert worst(got, ref) <= FLOOR_FACTOR * replicated["floor"]


def test_scale_invariance(base, replicated):
    data, _, s = base
    s = s + 0.5 * (s > 1)          # not only integers
    eng_1 = build_engine(data, cfg_for(), device="cpu", weights=s)
    eng_2 = build_engine(data, cfg_for(), device="cpu", weights=2 * s)
    assert eng_2.n_total == 2 * eng_1.n_total
    a, b = collect(eng_1), collect(eng_2)
    tol = FLOOR_FACTOR * replicated["floor"]
    assert worst(b, a, ("means", "R", "pi")) <= tol
    assert reldiff(b["N"] / 2, a["N"]) <= tol


def test_zero_weight_events_keep_posteriors(base):
    """Weight 0 removes an event from the fit, not from the output."""
    data, _, s = base
    eng = build_engine(data, cfg_for(), device="cpu", weights=s)
    eng.run_em(K)
    post = eng.posteriors(K)
    assert torch.allclose(post.sum(dim=0), torch.ones(N_BASE), atol=1e-5)
    w = eng.recompute_memberships(eng.state.shrink(K))
    assert w.shape == (K, N_BASE)
    assert torch.allclose(w.sum(dim=0), torch.ones(N_BASE), atol=1e-5)


def test_cpu_twin_of_kernel():
    lse = torch.tensor([-3.0, float("-inf"), 2.5, -1.0])
    s = torch.tensor([2.0, 0.0, 0.5, 0.0])
    lse_w, lik = cpu.event_weight_lse(lse, s, torch.log(s))
    assert lse_w[1] == float("inf") and lse_w[3] == float("inf")
    assert torch.equal(lse_w[[0, 2]], (lse - torch.log(s))[[0, 2]])
    assert float(lik) == 2.0 * -3.0 + 0.5 * 2.5
    logw = torch.log(torch.tensor([[0.25, 0.5, 0.1, 0.9],
                                   [0.75, 0.5, 0.9, 0.1]]))
    w, w_s, lik2 = cpu.estep_posteriors_weighted(logw, s)
    assert torch.allclose(w.sum(dim=0), torch.ones(4))
    assert torch.allclose(w_s.sum(dim=0), s)
    assert torch.equal(w_s[:, 1], torch.zeros(2))


@pytest.mark.parametrize("bad", ["negative", "nan", "length", "zero"])
def test_weight_validation(base, bad):
    data = base[0]
    w = np.ones(N_BASE, np.float32)
    if bad == "negative":
        w[7] = -1.0
    elif bad == "nan":
        w[7] = np.nan
    elif bad == "length":
        w = w[:-1]
    else:
        w[:] = 0.0
    with pytest.raises(ValueError):
        build_engine(data, cfg_for(), device="cpu", weights=w)


def test_scatter_input_with_weights_is_refused(base):
    from cuda_gmm_mpi_amd.engine import build_engine_sharded
    data = torch.from_numpy(base[0])
    with pytest.raises(ValueError, match="scatter"):
        build_engine_sharded(data, cfg_for(), N_BASE, data.mean(dim=0),
                             data.var(dim=0), data[:K],
                             weights=np.ones(N_BASE, np.float32))


def _cli_files(tmp_path, base, weights):
    from cuda_gmm_mpi_amd.utils import io as gio
    binpath = str(tmp_path / "d.bin")
    gio.write_bin(binpath, base[0])
    wpath = str(tmp_path / "w.bin")
    gio.write_bin(wpath, weights)
    return binpath, wpath


def test_cli_wrong_shaped_weights_is_usage_error(tmp_path, base, capsys):
    from cuda_gmm_mpi_amd.cli import main
    args = ["--min-iters", "2", "--max-iters", "2", "--device", "cpu"]
    out = str(tmp_path / "o")
    # two columns
    binpath, wpath = _cli_files(tmp_path, base,
                                np.ones((N_BASE, 2), np.float32))
    assert main(["3", binpath, out, "3", "--weights", wpath] + args) == 1
    # wrong length
    binpath, wpath = _cli_files(tmp_path, base,
                                np.ones((N_BASE - 1, 1), np.float32))
    assert main(["3", binpath, out, "3", "--weights", wpath] + args) == 1
    assert "Invalid weights file" in capsys.readouterr().out
    # scattering weights is out of scope
    assert main(["3", binpath, out, "3", "--weights", wpath,
                 "--scatter-input"] + args) == 1


def test_cli_round_trip(tmp_path, base):
    from cuda_gmm_mpi_amd.cli import main
    from cuda_gmm_mpi_amd.models.model import GmmModel
    from cuda_gmm_mpi_amd.utils import io as gio
    s = base[2] * 0.75
    binpath, wpath = _cli_files(tmp_path, base, s.reshape(-1, 1))
    out = str(tmp_path / "o")
    model_path = str(tmp_path / "m.npz")
    rc = main(["3", binpath, out, "3", "--weights", wpath, "--min-iters",
               "4", "--max-iters", "4", "--device", "cpu", "--save-model",
               model_path])
    assert rc == 0
    summary = gio.read_summary(out + ".summary")
    # %f prints 6 decimals; fp32 N of a few hundred carries ~3e-5 each
    total = float(s.astype(np.float64).sum())
    assert float(summary["N"].astype(np.float64).sum()) == pytest.approx(
        total, abs=1e-3 * K)
    model = GmmModel.load(model_path)
    assert float(np.asarray(model.N, np.float64).sum()) == pytest.approx(
        total, abs=1e-3 * K)
    # every event keeps its .results row, zero-weight ones included
    lines = open(out + ".results").read().splitlines()
    assert len(lines) == N_BASE
    zero_row = int(np.nonzero(s == 0)[0][0])
    post = [float(v) for v in lines[zero_row].split("\t")[1].split(",")]
    assert sum(post) == pytest.approx(1.0, abs=1e-4)


# ------------------------------------------------------------ world 2, gloo

def _fit_weighted():
    from cuda_gmm_mpi_amd.utils.synthetic import make_blobs
    data, _ = make_blobs(2002, 3, 3, seed=17)  # non-divisible N
    s = np.random.default_rng(3).choice(
        np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=2002)
    # avgvar ~ 0: the G*avgvar regularization is world-size dependent by
    # design, as in the unweighted gloo tests
    cfg = GmmConfig(num_clusters=3, target_num_clusters=3, min_iters=8,
                    max_iters=8, covariance_dynamic_range=1e15)
    eng = build_engine(data, cfg, device="cpu", weights=s)
    lik = eng.run_em(3)
    w = eng.recompute_memberships(eng.state.shrink(3))
    gathered = eng.gather_memberships(w)
    return {"lik": lik, "n_total": eng.n_total,
            "n_events_total": eng.n_events_total,
            "rows": None if gathered is None else gathered.shape[1],
            "means": eng.state.means.numpy().copy(),
            "R": eng.state.R.numpy().copy(),
            "N": eng.state.N.numpy().copy(),
            "pi": eng.state.pi.numpy().copy()}


def _worker(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world))
    import torch.distributed as dist
    from cuda_gmm_mpi_amd.parallel import dist as pdist
    pdist.init_process_group(backend="gloo")
    try:
        result = _fit_weighted()
        if rank == 0:
            out_q.put(result)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_weighted_matches_single_process():
    single = _fit_weighted()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29871, q))
             for r in range(2)]
    for p in procs:
        p.start()
    multi = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert multi["n_total"] == single["n_total"]
    assert multi["n_events_total"] == single["n_events_total"] == 2002
    assert multi["rows"] == 2002
    # the tolerances of test_dist_gloo's unweighted world-2 EM test
    assert multi["lik"] == pytest.approx(single["lik"], rel=1e-4)
    np.testing.assert_allclose(multi["N"], single["N"], rtol=1e-3)
    np.testing.assert_allclose(multi["means"], single["means"],
                               rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(multi["R"], single["R"], rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(multi["pi"], single["pi"], rtol=1e-3)
