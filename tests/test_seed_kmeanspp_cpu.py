"""Greedy k-means++ seeding on the CPU: the float64 host implementation
against a literal transcription of its contract, what it buys on data whose
rows are in arbitrary order, weights, and the plumbing (config, engine, CLI,
world 2 over gloo with and without --scatter-input)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from cuda_gmm_mpi_amd.cli import main
from cuda_gmm_mpi_amd.engine import build_engine
from cuda_gmm_mpi_amd.models.seed import (seed_indices_strided,
                                          seed_means_kmeanspp)
from cuda_gmm_mpi_amd.ops import functional as F
from cuda_gmm_mpi_amd.utils import io as gio
from cuda_gmm_mpi_amd.utils.config import GmmConfig
from cuda_gmm_mpi_amd.utils.synthetic import make_blobs, make_supported_blobs

# (N, D, K): the shapes of the issue's table; strided seeds on the shuffled
# rows hit 11, 7 and 4 distinct clusters
SHUFFLED_SHAPES = [(3001, 24, 16), (2500, 40, 12), (4096, 5, 8)]


def shuffled_blobs(n, d, k):
    """make_supported_blobs with the rows re-shuffled: the generator arranges
    its rows so that the strided seeds hit every cluster; a real file does
    not."""
    data, labels = make_supported_blobs(n, d, k, seed=3)
    perm = np.random.default_rng(11).permutation(n)
    return data[perm], labels[perm]


# ------------------------------------------------------------------ contract

def contract_seeds(x, k, seed_rng, s=None):
    """The contract, written out event by event in Python floats (float64):
    returns (indices, candidates per round, winning slot per round)."""
    x = [[float(v) for v in row] for row in np.asarray(x)]
    n = len(x)
    s = [1.0] * n if s is None else [float(v) for v in s]
    nl = 2 + math.floor(math.log(k))
    u = np.random.default_rng(seed_rng).random((k, 8))

    def pick(p, uu):
        total = 0.0
        for v in p:
            total += v
        run = 0.0
        for e, v in enumerate(p):
            run += v
            if run > uu * total:
                return e
        return n - 1

    def dist2(c):
        return [sum((a - b) * (a - b) for a, b in zip(row, x[c]))
                for row in x]

    i0 = pick(s, float(u[0, 0]))
    m = dist2(i0)
    indices, cands, winners = [i0], [[i0]], [0]
    for t in range(1, k):
        p = [a * b for a, b in zip(s, m)]
        if sum(p) == 0.0:
            p = s
        row, best = [], None
        for l in range(nl):
            c = pick(p, float(u[t, l]))
            dl = [min(a, b) for a, b in zip(m, dist2(c))]
            pot = math.fsum(a * b for a, b in zip(s, dl))
            row.append(c)
            if best is None or pot < best[0]:
                best = (pot, l, dl)
        m = best[2]
        cands.append(row)
        winners.append(best[1])
        indices.append(row[best[1]])
    return indices, cands, winners


def check_contract(x, k, seed_rng, s=None):
    means, idx, trace = seed_means_kmeanspp(x, k, seed_rng, weights=s)
    want_idx, want_cands, want_win = contract_seeds(x, k, seed_rng, s)
    nl = 2 + math.floor(math.log(k))
    assert idx.dtype == torch.int64 and idx.tolist() == want_idx
    assert trace["candidates"].shape == (k, nl)
    assert trace["candidates"][0].tolist() == want_cands[0] + [-1] * (nl - 1)
    for t in range(1, k):
        assert trace["candidates"][t].tolist() == want_cands[t]
    assert trace["winner"].tolist() == want_win
    assert means.dtype == torch.float32
    assert torch.equal(means, torch.as_tensor(np.asarray(x, np.float32))[idx])
    return idx


@pytest.mark.parametrize("n,d,k,seed_rng", [
    (97, 3, 5, 0), (64, 1, 4, 1), (33, 7, 1, 2), (150, 2, 9, 3)])
def test_contract_random(n, d, k, seed_rng):
    """Small random data, D = 1 and K = 1 included."""
    x = np.random.default_rng(100 + n).normal(size=(n, d)).astype(np.float32)
    x = (250.0 * x).astype(np.float32)
    check_contract(x, k, seed_rng)


def test_contract_zero_potential_branch():
    """N = 5 with 3 distinct rows and K = 4: after three picks every
    distance is 0 and the last round draws from the weights alone."""
    a, b, c = [1.0, 2.0], [30.0, -4.0], [-7.0, 9.0]
    x = np.array([a, b, a, c, b], dtype=np.float32)
    for seed_rng in range(6):
        idx = check_contract(x, 4, seed_rng)
        assert len({tuple(x[i]) for i in idx.tolist()}) == 3


def test_contract_weighted():
    rng = np.random.default_rng(5)
    x = (250.0 * rng.normal(size=(120, 4))).astype(np.float32)
    s = rng.integers(0, 4, size=120).astype(np.float32)
    idx = check_contract(x, 6, 4, s)
    assert (s[idx.numpy()] > 0).all()


# --------------------------------------------------------- distinct clusters

@pytest.mark.parametrize("n,d,k", SHUFFLED_SHAPES)
def test_distinct_clusters_on_shuffled_rows(n, d, k):
    data, labels = shuffled_blobs(n, d, k)
    _, idx, _ = seed_means_kmeanspp(data, k, 0)
    assert len(set(labels[idx.numpy()].tolist())) == k
    # the gap this closes: the strided rows of the same file miss clusters
    strided = seed_indices_strided(n, k).numpy()
    assert len(set(labels[strided].tolist())) < k


# ------------------------------------------------------------------- weights

def test_mask_gives_the_seeds_of_the_subset():
    data, _ = shuffled_blobs(3001, 24, 16)
    mask = (np.random.default_rng(2).random(3001) < 0.6).astype(np.float32)
    kept = np.nonzero(mask > 0)[0]
    _, idx_w, _ = seed_means_kmeanspp(data, 16, 0, weights=mask)
    _, idx_s, _ = seed_means_kmeanspp(data[kept], 16, 0)
    assert idx_w.tolist() == kept[idx_s.numpy()].tolist()
    assert (mask[idx_w.numpy()] > 0).all()


def test_integer_weights_give_the_seeds_of_the_replicated_file():
    data, _ = shuffled_blobs(3001, 24, 16)
    s = np.random.default_rng(3).integers(0, 4, size=3001)
    rows = np.repeat(np.arange(3001), s)
    _, idx_w, _ = seed_means_kmeanspp(data, 16, 0,
                                      weights=s.astype(np.float32))
    _, idx_r, _ = seed_means_kmeanspp(data[rows], 16, 0)
    assert idx_w.tolist() == rows[idx_r.numpy()].tolist()
    assert (s[idx_w.numpy()] > 0).all()


# -------------------------------------------------------- config / dispatch

def test_config_validation():
    GmmConfig(num_clusters=3, seed_method="kmeans++", seed_rng=7).validate()
    assert GmmConfig().seed_method == "strided" and GmmConfig().seed_rng == 0
    for bad in (dict(seed_method="kmeans"), dict(seed_method=""),
                dict(seed_rng=-1), dict(seed_rng=1.5), dict(seed_rng="0"),
                dict(seed_rng=True)):
        with pytest.raises(ValueError):
            GmmConfig(num_clusters=3, **bad).validate()


def test_functional_cpu_dispatch():
    data, _ = make_blobs(300, 3, 4, seed=9)
    means, idx, trace = F.seed_kmeanspp(data, 4, 5, device="cpu")
    ref_means, ref_idx, ref_trace = seed_means_kmeanspp(data, 4, 5)
    assert torch.equal(idx, ref_idx) and torch.equal(means, ref_means)
    assert torch.equal(trace["candidates"], ref_trace["candidates"])


def test_distribute_input_seed_arguments_default_to_strided():
    """World 1: without the new arguments the strided seeds, with them the
    caller's seeding and its rows."""
    from cuda_gmm_mpi_amd.engine import seed_full_data
    from cuda_gmm_mpi_amd.models.seed import seed_means_host
    from cuda_gmm_mpi_amd.parallel import dist as pdist
    data, _ = make_blobs(500, 3, 4, seed=21)
    full = torch.from_numpy(data)
    out = pdist.distribute_input(full, 4)
    assert len(out) == 5 and torch.equal(out[4], seed_means_host(full, 4))
    cfg = GmmConfig(num_clusters=4, seed_method="kmeans++", seed_rng=2)
    info = {}
    out = pdist.distribute_input(
        full, 4, seed_fn=lambda d: seed_full_data(d, cfg, "cpu"),
        seed_info=info)
    means, idx, _ = seed_means_kmeanspp(data, 4, 2)
    assert torch.equal(out[4], means) and torch.equal(info["indices"], idx)


# -------------------------------------------------------------------- engine

def test_engine_kmeanspp_beats_strided_on_shuffled_rows():
    """(3001, 24, 16), 100 EM iterations at K0 = K: seeding every cluster
    ends at a likelihood at least as high (measured -334417 vs -337453)."""
    data, _ = shuffled_blobs(3001, 24, 16)
    lik = {}
    for method in ("strided", "kmeans++"):
        cfg = GmmConfig(num_clusters=16, target_num_clusters=16,
                        seed_method=method, seed_rng=0)
        eng = build_engine(data, cfg, device="cpu")
        lik[method] = eng.run_em(16)
        if method == "kmeans++":
            _, idx, _ = seed_means_kmeanspp(data, 16, 0)
            assert eng.seed_indices == idx.tolist()
        else:
            assert eng.seed_indices == seed_indices_strided(3001, 16).tolist()
    print(lik)
    assert lik["kmeans++"] >= lik["strided"]


def test_engine_weighted_kmeanspp_never_seeds_a_zero_weight_event():
    data, _ = shuffled_blobs(3001, 24, 16)
    s = np.random.default_rng(3).integers(0, 3, size=3001).astype(np.float32)
    cfg = GmmConfig(num_clusters=16, target_num_clusters=16, min_iters=1,
                    max_iters=1, seed_method="kmeans++", seed_rng=0)
    eng = build_engine(data, cfg, device="cpu", weights=s)
    _, idx, _ = seed_means_kmeanspp(data, 16, 0, weights=s)
    assert eng.seed_indices == idx.tolist()
    assert (s[eng.seed_indices] > 0).all()


# ----------------------------------------------------------------------- CLI

CLI_TAIL = ["--min-iters", "4", "--max-iters", "4", "--device", "cpu",
            "--no-results", "--covariance-dynamic-range", "1e15"]


@pytest.fixture(scope="module")
def cli_file(tmp_path_factory):
    work = tmp_path_factory.mktemp("seedcli")
    data, _ = shuffled_blobs(1507, 3, 4)
    gio.write_bin(str(work / "data.bin"), data)
    return work, data


def test_cli_strided_flag_is_the_default_run(cli_file):
    work, _ = cli_file
    binp = str(work / "data.bin")
    assert main(["4", binp, str(work / "plain"), "3"] + CLI_TAIL) == 0
    assert main(["4", binp, str(work / "flag"), "3", "--seed-method",
                 "strided"] + CLI_TAIL) == 0
    plain = open(work / "plain.summary", "rb").read()
    assert plain and plain == open(work / "flag.summary", "rb").read()


def test_cli_kmeanspp_round_trip(cli_file):
    work, data = cli_file
    binp = str(work / "data.bin")
    mpath = str(work / "m.json")
    assert main(["4", binp, str(work / "kpp"), "3", "--seed-method",
                 "kmeans++", "--seed", "0", "--metrics-out", mpath]
                + CLI_TAIL) == 0
    metrics = json.load(open(mpath))
    _, idx, _ = seed_means_kmeanspp(data, 4, 0)
    assert metrics["seed_method"] == "kmeans++" and metrics["seed_rng"] == 0
    assert metrics["seed_indices"] == idx.tolist()
    assert open(work / "kpp.summary").read().count("Cluster #") == 3
    # another seed, other starting rows; the same seed, the same file
    assert main(["4", binp, str(work / "kpp7"), "3", "--seed-method",
                 "kmeans++", "--seed", "7", "--metrics-out", mpath]
                + CLI_TAIL) == 0
    assert json.load(open(mpath))["seed_indices"] != idx.tolist()
    assert main(["4", binp, str(work / "kpp0"), "3", "--seed-method",
                 "kmeans++", "--seed", "0"] + CLI_TAIL) == 0
    assert (open(work / "kpp0.summary", "rb").read()
            == open(work / "kpp.summary", "rb").read())


def test_cli_rejects_bad_seed_arguments(cli_file):
    work, _ = cli_file
    binp = str(work / "data.bin")
    assert main(["4", binp, str(work / "bad"), "--seed-method", "random"]
                + CLI_TAIL) == 1
    assert main(["4", binp, str(work / "bad"), "--seed-method", "kmeans++",
                 "--seed", "-3"] + CLI_TAIL) == 1
    assert main(["4", binp, str(work / "bad"), "--seed", "x"] + CLI_TAIL) == 1


# ------------------------------------------------------------- gloo, world 2

def _worker(rank, world, port, fn_name, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["LOCAL_RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    import torch.distributed as dist
    from cuda_gmm_mpi_amd.parallel import dist as pdist
    pdist.init_process_group(backend="gloo")
    try:
        result = globals()[fn_name]()
        if rank == 0:
            out_q.put(result)
    finally:
        if dist.is_initialized():  # the CLI destroys the group itself
            dist.destroy_process_group()


def run_world(world, fn_name, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, fn_name, q))
             for r in range(world)]
    for p in procs:
        p.start()
    result = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return result


def _cli_kpp(scatter):
    work = os.environ["GMM_TEST_SEED_DIR"]
    rank = os.environ.get("RANK", "0")
    out = os.path.join(work, f"w2_{'sc' if scatter else 'fs'}_{rank}")
    mpath = out + ".json"
    argv = (["4", os.path.join(work, "data.bin"), out, "3", "--seed-method",
             "kmeans++", "--seed", "0", "--metrics-out", mpath] + CLI_TAIL)
    if scatter:
        argv.append("--scatter-input")
    assert main(argv) == 0
    if rank != "0":
        return None
    return {"summary": open(out + ".summary").read(),
            "indices": json.load(open(mpath))["seed_indices"]}


def _cli_kpp_scatter():
    return _cli_kpp(True)


def _cli_kpp_shared():
    return _cli_kpp(False)


@pytest.mark.timeout(300)
def test_world2_seeds_and_summary_equal_world1(cli_file):
    work, data = cli_file
    out = str(work / "w1")
    mpath = out + ".json"
    assert main(["4", str(work / "data.bin"), out, "3", "--seed-method",
                 "kmeans++", "--seed", "0", "--metrics-out", mpath]
                + CLI_TAIL) == 0
    single = {"summary": open(out + ".summary").read(),
              "indices": json.load(open(mpath))["seed_indices"]}
    os.environ["GMM_TEST_SEED_DIR"] = str(work)
    try:
        shared = run_world(2, "_cli_kpp_shared", port=29831)
        scattered = run_world(2, "_cli_kpp_scatter", port=29832)
    finally:
        os.environ.pop("GMM_TEST_SEED_DIR", None)
    _, idx, _ = seed_means_kmeanspp(data, 4, 0)
    assert single["indices"] == idx.tolist()
    assert shared["indices"] == scattered["indices"] == single["indices"]
    # the two world-2 paths agree byte for byte. Against world 1 the seeds
    # are identical and the fit differs by the shard order of its fp32
    # reductions alone (the world-size dependent avgvar ridge is switched
    # off, as in test_dist_gloo): same tolerances as that file's
    # world-2-against-single comparison
    assert shared["summary"] == scattered["summary"]
    print("world 2 == world 1 byte for byte:",
          shared["summary"] == single["summary"])
    got = gio.read_summary(str(work / "w2_fs_0.summary"))
    ref = gio.read_summary(out + ".summary")
    assert got["means"].shape == ref["means"].shape == (3, 3)
    np.testing.assert_allclose(got["N"], ref["N"], rtol=1e-3)
    np.testing.assert_allclose(got["pi"], ref["pi"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(got["means"], ref["means"],
                               rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(got["R"], ref["R"], rtol=2e-2, atol=2e-2)
