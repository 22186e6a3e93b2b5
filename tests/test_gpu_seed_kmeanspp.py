"""Greedy k-means++ seeding kernels (seed_kmeanspp.hip) on the GPU.

The stages are checked one by one against float64 (distances, scratch rows,
m, block partials, winner), whole seedings by replaying the device's own
trace on the host: the GPU draws from fp32 distances, so its picks need not
equal the CPU's, but every candidate must lie in the interval its uniform
selects (within the rounding of the cumulative mass) and every winner must
attain the round's minimum potential.

Tolerances: a distance is D products of fp32 differences summed in fp32, so
its relative error is within TOL(D) = 4 D 2^-24 (D roundings of the products,
D of the additions, the differences themselves, plus margin). The float64
block sums are compared with the float64 sum of the device's own fp32 values
within n 2^-52 relative.
"""
import math

import numpy as np
import pytest
import torch

from cuda_gmm_mpi_amd.models.seed import (kmeanspp_num_candidates,
                                          kmeanspp_uniforms,
                                          seed_indices_strided)
from cuda_gmm_mpi_amd.ops import functional as F
from cuda_gmm_mpi_amd.utils.config import GmmConfig
from cuda_gmm_mpi_amd.utils.synthetic import make_supported_blobs

pytestmark = pytest.mark.gpu

SHUFFLED_SHAPES = [(3001, 24, 16), (2500, 40, 12), (4096, 5, 8)]
STAGES_NO_SAMPLE = F.SEED_EVALUATE | F.SEED_CHOOSE | F.SEED_COMMIT


def tol(d):
    return 4.0 * d * 2.0 ** -24


def random_data(n, d, seed):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(50.0, 750.0, size=(5, d))
    x = centers[rng.integers(0, 5, size=n)] + 25.0 * rng.normal(size=(n, d))
    return x.astype(np.float32)


def shuffled_blobs(n, d, k):
    data, labels = make_supported_blobs(n, d, k, seed=3)
    perm = np.random.default_rng(11).permutation(n)
    return data[perm], labels[perm]


def dist2(x64, row):
    diff = x64 - x64[row]
    return np.einsum("ij,ij->i", diff, diff)


def workspace(x, k, seed_rng=0, s=None):
    return F.seed_kmeanspp_workspace(
        torch.from_numpy(x).cuda(), k, seed_rng,
        None if s is None else torch.from_numpy(s))


def assert_close_rel(got, ref, rel, what):
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > rel * np.abs(ref)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.size} beyond {rel:.3e} relative, "
        f"worst {float((err / np.maximum(np.abs(ref), 1e-300)).max()):.3e}")


# ------------------------------------------------------ evaluate / commit

STAGE_CASES = (
    [(n, d, 512, False) for n in (1, 63, 257, 3001)
     for d in (1, 24, 31, 32, 40)]
    + [(600, 24, 2, False), (600, 24, 512, True), (600, 24, 2, True),
       (3001, 40, 16, True)])


@pytest.mark.parametrize("n,d,k,weighted", STAGE_CASES)
def test_evaluate_choose_commit(n, d, k, weighted):
    """Round 0 and one later round with caller-written candidates, among
    them the row chosen in round 0 and a repeated row (distance 0)."""
    x = random_data(n, d, 1000 + n + d)
    x64 = x.astype(np.float64)
    rng = np.random.default_rng(n * 131 + d)
    s = (rng.integers(0, 4, size=n).astype(np.float32) if weighted else None)
    s64 = np.ones(n) if s is None else s.astype(np.float64)
    nl = kmeanspp_num_candidates(k)
    assert nl == (2 if k == 2 else 8 if k == 512 else 4)
    ws = workspace(x, k, 0, s)
    nblk = (n + 255) // 256
    assert ws["pot_part"].shape == (nblk, 8)

    # round 0: one candidate, m does not exist yet
    i0 = n // 3
    ws["cand"][0] = i0
    F.seed_kmeanspp_rounds(ws, 0, 1, STAGES_NO_SAMPLE)
    torch.cuda.synchronize()
    m0 = ws["m"].cpu().numpy()
    ref0 = dist2(x64, i0)
    assert_close_rel(m0, ref0, tol(d), "round 0 m")
    assert m0[i0] == 0.0
    assert np.array_equal(ws["scratch"][0].cpu().numpy(), m0)
    assert int(ws["winner"][0]) == 0 and int(ws["index"][0]) == i0
    own = float(np.sum(s64 * m0.astype(np.float64)))
    for name, got in (("pot_part", float(ws["pot_part"][:, 0].sum())),
                      ("pots", float(ws["pots"][0, 0])),
                      ("sm_part", float(ws["sm_part"].sum()))):
        print(f"round 0 {name}: {got!r} vs {own!r}")
        assert abs(got - own) <= n * 2.0 ** -52 * own, name
    if k == 1 or nl < 2:
        return

    # a later round: candidates with the chosen row and a repeat among them
    cands = rng.integers(0, n, size=nl)
    cands[0] = i0
    cands[nl - 1] = cands[1]
    ws["cand"][1, :nl] = torch.from_numpy(cands).cuda()
    ws["cand"][1, nl:] = int(cands[0])
    F.seed_kmeanspp_rounds(ws, 1, 2, STAGES_NO_SAMPLE)
    torch.cuda.synchronize()
    scratch = ws["scratch"].cpu().numpy()
    pots_dev = ws["pots"][1].cpu().numpy()
    part = ws["pot_part"].cpu().numpy().sum(axis=0)
    for l in range(nl):
        ref = np.minimum(ref0, dist2(x64, int(cands[l])))
        assert_close_rel(scratch[l], ref, tol(d), f"scratch row {l}")
        assert scratch[l][cands[l]] == 0.0 and scratch[l][i0] == 0.0
        own = float(np.sum(s64 * scratch[l].astype(np.float64)))
        print(f"slot {l}: potential {pots_dev[l]!r} vs {own!r}")
        assert abs(part[l] - own) <= n * 2.0 ** -52 * own
        assert abs(pots_dev[l] - own) <= n * 2.0 ** -52 * own
    # slot 0 repeats the chosen row: it changes nothing and cannot win
    # unless every slot ties; the winner is the lowest slot of the minimum
    w = int(ws["winner"][1])
    assert w == int(np.argmin(pots_dev[:nl]))
    assert int(ws["index"][1]) == int(cands[w])
    m1 = ws["m"].cpu().numpy()
    assert np.array_equal(m1, scratch[w])
    own = float(np.sum(s64 * m1.astype(np.float64)))
    assert abs(float(ws["sm_part"].sum()) - own) <= n * 2.0 ** -52 * own


def test_unaligned_rows_take_the_scalar_walk():
    """Full blocks of 16-byte aligned data are staged as vectors; the same
    rows at an address that is not (a view one row into a D = 5 buffer) go
    through the scalar walk and must give the very same bits."""
    x = random_data(1025, 5, 77)
    dev = torch.from_numpy(x).cuda()
    view = dev[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    results = []
    for xd in (view, view.clone()):
        ws = F.seed_kmeanspp_workspace(xd, 8, 1)
        F.seed_kmeanspp_rounds(ws, 0, 8)
        results.append((ws["index"].cpu(), ws["m"].cpu(), ws["pots"].cpu()))
    assert results[1][0].tolist() != [0] * 8
    for a, b in zip(*results):
        assert torch.equal(a, b)


# ------------------------------------------------------------ trace replay

def replay(x, k, seed_rng, s, idx, trace):
    """Replay a device trace in float64 from the device's own winners."""
    n, d = x.shape
    x64 = x.astype(np.float64)
    s64 = np.ones(n) if s is None else s.astype(np.float64)
    nl = kmeanspp_num_candidates(k)
    u = kmeanspp_uniforms(k, seed_rng)
    cands = trace["candidates"].numpy()
    winner = trace["winner"].numpy()
    idx = idx.numpy()
    assert cands.shape == (k, nl) and winner.shape == (k,)

    def check_pick(p, c, uu, what):
        assert 0 <= c < n, what
        assert p[c] > 0.0, f"{what}: picked an event without mass"
        cum = np.cumsum(p)
        total = cum[-1]
        tau = tol(d) * total
        lo = cum[c - 1] if c > 0 else 0.0
        assert lo - tau <= uu * total < cum[c] + tau, (
            f"{what}: row {c} covers [{lo!r}, {cum[c]!r}) of {total!r}, "
            f"uniform asks for {uu * total!r}")

    i0 = int(cands[0, 0])
    check_pick(s64, i0, u[0, 0], "round 0")
    assert (cands[0, 1:] == -1).all() and winner[0] == 0 and idx[0] == i0
    m = dist2(x64, i0)
    for t in range(1, k):
        p = s64 * m
        if p.sum() == 0.0:
            p = s64
        pots = np.empty(nl)
        for l in range(nl):
            c = int(cands[t, l])
            check_pick(p, c, u[t, l], f"round {t} slot {l}")
            pots[l] = np.sum(s64 * np.minimum(m, dist2(x64, c)))
        w = int(winner[t])
        assert 0 <= w < nl
        assert pots[w] <= pots.min() * (1.0 + tol(d)), (
            f"round {t}: slot {w} has {pots[w]!r}, minimum {pots.min()!r}")
        assert idx[t] == cands[t, w]
        m = np.minimum(m, dist2(x64, int(idx[t])))


REPLAY_CASES = [
    # n, d, k, weighted
    (600, 24, 2, False),       # L = 2
    (600, 24, 512, False),     # L = 8, all but 88 rows end up chosen
    (1, 5, 3, False),          # a single event: every pick is row 0
    (63, 32, 4, True),         # below one wave
    (257, 31, 8, False),       # one event past a block
    (3001, 24, 16, True),
    (3001, 40, 12, False),
    (70001, 3, 4, False),      # more than 256 blocks: multi-block segments
]


@pytest.mark.parametrize("n,d,k,weighted", REPLAY_CASES)
def test_replay_of_the_device_trace(n, d, k, weighted):
    x = random_data(n, d, 2000 + n + d)
    s = (np.random.default_rng(n).integers(0, 4, size=n).astype(np.float32)
         if weighted else None)
    means, idx, trace = F.seed_kmeanspp(x, k, 3, weights=s, device="cuda")
    assert torch.equal(means, torch.from_numpy(x)[idx])
    replay(x, k, 3, s, idx, trace)
    if s is not None:
        assert (s[idx.numpy()] > 0).all()


def test_replay_zero_potential_branch():
    """5 rows, 3 distinct, K = 4: the last round has no potential left and
    draws from the weights."""
    a, b, c = [1.0, 2.0], [30.0, -4.0], [-7.0, 9.0]
    x = np.array([a, b, a, c, b], dtype=np.float32)
    for seed_rng in range(4):
        _, idx, trace = F.seed_kmeanspp(x, 4, seed_rng, device="cuda")
        assert len({tuple(x[i]) for i in idx.tolist()}) == 3
        replay(x, 4, seed_rng, None, idx, trace)


# ------------------------------------------------------------ other checks

@pytest.mark.parametrize("n,d,k", SHUFFLED_SHAPES)
def test_distinct_clusters_on_shuffled_rows(n, d, k):
    data, labels = shuffled_blobs(n, d, k)
    _, idx, trace = F.seed_kmeanspp(data, k, 0, device="cuda")
    hit = labels[idx.numpy()]
    print("indices", idx.tolist(), "labels", hit.tolist())
    print("candidates", trace["candidates"].tolist())
    assert len(set(hit.tolist())) == k
    assert len(set(labels[seed_indices_strided(n, k).numpy()].tolist())) < k


def test_two_runs_are_bit_identical():
    x = random_data(3001, 24, 7)
    s = np.random.default_rng(8).integers(0, 3, size=3001).astype(np.float32)
    runs = []
    for _ in range(2):
        ws = workspace(x, 16, 5, s)
        F.seed_kmeanspp_rounds(ws, 0, 16)
        runs.append((ws["index"].cpu(), ws["m"].cpu(), ws["cand"].cpu(),
                     ws["pots"].cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert (s[runs[0][0].numpy()] > 0).all()


def test_cli_on_one_gpu(tmp_path):
    """gmm 16 shuffled.bin out 16 --seed-method kmeans++ --seed 0 on cuda:
    the seeds in the metrics are the device's own draw for that seed."""
    import json
    from cuda_gmm_mpi_amd.cli import main
    from cuda_gmm_mpi_amd.utils import io as gio
    data, labels = shuffled_blobs(3001, 24, 16)
    gio.write_bin(str(tmp_path / "shuffled.bin"), data)
    mpath = str(tmp_path / "m.json")
    assert main(["16", str(tmp_path / "shuffled.bin"), str(tmp_path / "out"),
                 "16", "--seed-method", "kmeans++", "--seed", "0",
                 "--min-iters", "5", "--max-iters", "5", "--device", "cuda",
                 "--no-results", "--metrics-out", mpath]) == 0
    metrics = json.load(open(mpath))
    _, idx, _ = F.seed_kmeanspp(data, 16, 0, device="cuda")
    assert metrics["seed_method"] == "kmeans++" and metrics["seed_rng"] == 0
    assert metrics["seed_indices"] == idx.tolist()
    assert len(set(labels[metrics["seed_indices"]].tolist())) == 16
    assert open(tmp_path / "out.summary").read().count("Cluster #") == 16


@pytest.mark.parametrize("estep_dtype", ["bf16", "fp32"])
def test_engine_kmeanspp_beats_strided_on_shuffled_rows(estep_dtype):
    from cuda_gmm_mpi_amd.engine import build_engine
    data, _ = shuffled_blobs(3001, 24, 16)
    lik = {}
    for method in ("strided", "kmeans++"):
        cfg = GmmConfig(num_clusters=16, target_num_clusters=16,
                        seed_method=method, seed_rng=0,
                        estep_dtype=estep_dtype)
        eng = build_engine(data, cfg, device="cuda")
        lik[method] = eng.run_em(16)
        assert len(eng.seed_indices) == 16
    print(estep_dtype, lik)
    assert math.isfinite(lik["kmeans++"])
    assert lik["kmeans++"] >= lik["strided"]
