"""Uniform background component on the CPU engine path: the float64 oracle
of background_oracle.py and its fp32 twins, the engine on the blobs-plus-
noise dataset against the oracle's EM loop, weights, the MDL score and
sweep, model files, the command line and a gloo world of 2.

The fitted mixture is (1 - pi0) sum_c pi_c N_c(x) + pi0 / V; everything
printed before an assertion is the measured figure next to its bound.
"""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import background_oracle as bo

from cuda_gmm_mpi_amd.engine import EmEngine, build_engine
from cuda_gmm_mpi_amd.models.model import GmmModel
from cuda_gmm_mpi_amd.ops import cpu_reference as cpu
from cuda_gmm_mpi_amd.ops import functional as F
from cuda_gmm_mpi_amd.utils import io as gio
from cuda_gmm_mpi_amd.utils.config import GmmConfig, rissanen_score

INF = float("inf")
U32 = 2.0 ** -24


def cfg_for(k, iters, **kw):
    return GmmConfig(num_clusters=k, target_num_clusters=k,
                     min_iters=iters, max_iters=iters, **kw)


# ------------------------------------------------------------------ oracle
def lse_case(n=257, seed=3):
    rng = np.random.default_rng(seed)
    lse = (rng.standard_normal(n) * 20 - 30).astype(np.float32)
    lse[n // 2] = -INF
    s = rng.choice(np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=n)
    return lse, s


def test_oracle_b_minus_inf_is_identity():
    lse, s = lse_case()
    lse_b, lse_m, n0, lik = bo.background_lse(lse, -INF)
    assert np.array_equal(lse_b, lse.astype(np.float64))
    assert np.array_equal(lse_m, lse_b) and n0 == 0.0
    lse_b, lse_m, n0, _ = bo.background_lse(lse, -INF, s)
    assert np.array_equal(lse_b, lse.astype(np.float64)) and n0 == 0.0
    assert (lse_m[s == 0] == INF).all()
    # both -inf -> -inf; a finite b lifts it to b with r0 = 1
    assert lse_b[len(lse) // 2] == -INF
    assert bo.background_lse(lse, -40.0)[0][len(lse) // 2] == -40.0


def test_oracle_posteriors_and_r0_sum_to_one():
    rng = np.random.default_rng(4)
    logw = rng.uniform(-60.0, 0.0, (4, 300))
    m = logw.max(axis=0)
    lse = m + np.log(np.exp(logw - m).sum(axis=0))
    for b in (-80.0, -30.0, 5.0):
        lse_b, _, n0, _ = bo.background_lse(lse, b)
        r0 = np.exp(b - lse_b)
        total = np.exp(logw - lse_b).sum(axis=0) + r0
        assert np.abs(total - 1.0).max() <= 1e-12
        assert n0 == pytest.approx(r0.sum(), rel=1e-14)


def test_oracle_update():
    assert bo.background_update(0.0, 100.0, 7.0) == (0.0, -INF, 0.0)
    pi0, b, add = bo.background_update(25.0, 100.0, 7.0)
    assert pi0 == 0.25 and b == pytest.approx(np.log(1 / 3) - 7.0)
    assert add == pytest.approx(100.0 * np.log(0.75))
    pi0, _, _ = bo.background_update(100.0, 100.0, 7.0)
    assert pi0 == 1.0 - 1e-6


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("b", [-INF, -35.0, 170.0])
def test_cpu_twins_agree_with_oracle(b, weighted):
    lse, s = lse_case()
    sw = s if weighted else None
    ref_b, ref_m, ref_n0, ref_lik = bo.background_lse(lse, b, sw)
    lse_t = torch.from_numpy(lse)
    got_b, got_m, n0, lik = cpu.background_lse(
        lse_t, b, torch.from_numpy(s) if weighted else None)
    fin = np.isfinite(ref_b)
    # one rounding of the sum plus a few ulp on a correction <= ln 2
    tol = 4 * U32 * np.maximum(1.0, np.abs(ref_b[fin]))
    assert (np.abs(got_b.numpy()[fin] - ref_b[fin]) <= tol).all()
    assert np.array_equal(got_b.numpy()[~fin], ref_b[~fin])
    fin_m = np.isfinite(ref_m)
    assert np.array_equal(np.isposinf(got_m.numpy()), np.isposinf(ref_m))
    tol_m = 6 * U32 * np.maximum(1.0, np.abs(ref_m[fin_m]))
    assert (np.abs(got_m.numpy()[fin_m] - ref_m[fin_m]) <= tol_m).all()
    if b == -INF:
        assert torch.equal(got_b, lse_t) and float(n0) == 0.0
    live = np.ones_like(lse, bool) if sw is None else s > 0
    if np.isfinite(ref_lik):
        n = len(lse)
        assert abs(float(n0) - ref_n0) <= n * U32 * max(ref_n0, 1.0)
        scale = np.abs(ref_b[live] * (1 if sw is None else s[live])).sum()
        assert abs(float(lik) - ref_lik) <= n * U32 * scale
    # the functional wrapper on CPU tensors is the same twin
    bg = torch.tensor([0.5, b, 0.0, 0.0])
    part = F.background_partial(len(lse), "cpu")
    out_m, out_b = torch.empty_like(lse_t), torch.empty_like(lse_t)
    F.background_lse(lse_t, bg, torch.from_numpy(s) if weighted else None,
                     torch.log(torch.from_numpy(s)) if weighted else None,
                     out_m, part, lse_b=out_b)
    assert torch.equal(out_m, got_m) and torch.equal(out_b, got_b)
    assert float(part[0, 0]) == float(n0)


@pytest.mark.parametrize("n0,n_total", [(0.0, 50.0), (3.5, 50.0),
                                        (50.0, 50.0), (80.0, 50.0)])
def test_update_twin_agrees_with_oracle(n0, n_total):
    ref = bo.background_update(n0, n_total, 12.5)
    got = cpu.background_update(n0, n_total, 12.5)
    assert got == pytest.approx(ref, rel=1e-15)
    bg = F.background_state("cpu")
    assert bg.tolist() == [0.0, -INF, 0.0, 0.0]
    F.background_update(torch.tensor([n0 / 2, n0 / 2]), n_total, 12.5, bg)
    want = np.array(list(ref) + [n0], dtype=np.float32)
    assert np.array_equal(bg.numpy(), want)


def test_log_volume():
    data = np.array([[0.0, 1.0], [2.0, 5.0], [1.0, 3.0], [9.0, 9.0]])
    assert F.background_log_volume(data) == pytest.approx(
        np.log(9.0) + np.log(8.0))
    # events with weight 0 do not span the box
    assert F.background_log_volume(data, np.array([1, 1, 1, 0.0])) == \
        pytest.approx(np.log(2.0) + np.log(4.0))
    flat = data.copy()
    flat[:, 1] = 3.0
    with pytest.raises(ValueError, match="dimension 1"):
        F.background_log_volume(flat)


# ---------------------------------------------- engine, prototype dataset
@pytest.fixture(scope="module")
def proto():
    """D = 20, 3 x 2000 blob events + 600 uniform noise events, scale 100,
    and the float64 oracle fit (computed once)."""
    data, labels = bo.blobs_plus_noise(0)
    assert data.shape == (6600, 20)
    rows = bo.seed_rows(6600, 3)
    # the precondition of the comparison: one seed per blob
    assert sorted(labels[rows].tolist()) == [0, 1, 2]
    ref = bo.em_fit(data, 3, 30)
    blob_trace = max(
        float(np.trace(np.cov(data[labels == c].astype(np.float64).T)))
        for c in range(3))
    return {"data": data, "labels": labels, "ref": ref,
            "blob_trace": blob_trace}


@pytest.fixture(scope="module")
def proto_fit(proto):
    eng = build_engine(proto["data"], cfg_for(3, 30, background=True),
                       device="cpu")
    lik = eng.run_em(3)
    return eng, lik


def test_oracle_loop_reproduces_the_prototype(proto):
    ref, labels = proto["ref"], proto["labels"]
    assert abs(ref["pi0"] - 600 / 6600) <= 1e-3
    r0 = ref["post"][3]
    assert (r0[labels == -1] > 0.5).all() and not (r0[labels >= 0] > 0.5).any()


def test_engine_recovers_noise_fraction_and_covariances(proto, proto_fit):
    eng, _ = proto_fit
    labels = proto["labels"]
    pi0 = eng.background_pi
    print(f"pi0 {pi0!r} (truth {600 / 6600!r}, oracle "
          f"{proto['ref']['pi0']!r}), N0 {eng.background_n!r}")
    assert abs(pi0 - 600 / 6600) <= 0.005
    post = eng.posteriors(3)
    assert post.shape == (4, 6600)
    assert float((post.sum(dim=0) - 1.0).abs().max()) <= 1e-5
    r0 = post[3].numpy()
    noise = float((r0[labels == -1] > 0.5).mean())
    blob = float((r0[labels >= 0] > 0.5).mean())
    print(f"r0 > 0.5: noise {noise:.4f}, blob {blob:.4f}")
    assert noise >= 0.95 and blob <= 0.01
    traces = [float(torch.trace(r)) for r in eng.state.R[:3]]
    print("traces / largest blob trace",
          [t / proto["blob_trace"] for t in traces])
    assert max(traces) <= 1.5 * proto["blob_trace"]
    # N_c + N0 account for every event
    assert float(eng.state.N[:3].sum()) + eng.background_n == pytest.approx(
        6600.0, rel=1e-5)


def test_without_background_one_cluster_swallows_the_noise(proto):
    """What the feature is for: the same fit without it."""
    eng = build_engine(proto["data"], cfg_for(3, 30), device="cpu")
    eng.run_em(3)
    assert eng._bg is None and eng._bg_partial is None and eng._lse_b is None
    traces = [float(torch.trace(r)) for r in eng.state.R[:3]]
    print("traces / largest blob trace",
          [t / proto["blob_trace"] for t in traces])
    assert max(traces) >= 5.0 * proto["blob_trace"]
    assert eng.posteriors(3).shape == (3, 6600)


def test_engine_matches_oracle_loop(proto, proto_fit):
    eng, lik = proto_fit
    ref = proto["ref"]
    rel = abs(lik - ref["lik"]) / abs(ref["lik"])
    print(f"likelihood fp32 {lik!r} float64 {ref['lik']!r} rel {rel:.3e}")
    # the relative allowance test_engine_cpu.py gives fp32 likelihoods
    # (1e-5 of |L|, its monotonicity and resume checks)
    assert rel <= 1e-5
    assert eng.likelihood == lik
    post = eng.posteriors(3).numpy()
    print("max |posterior - oracle|", np.abs(post - ref["post"]).max())
    assert np.abs(post - ref["post"]).max() <= 1e-3
    np.testing.assert_allclose(
        (eng.state.means[:3] + eng.center).numpy(), ref["means"],
        rtol=1e-4, atol=1e-2)


def test_warmup_zero_switches_on_after_first_estep(proto):
    """Warm-up 0 is the prototype's failure mode on FCS-scale data (the
    background takes every event), which is why the default is 5; here it
    only has to follow the schedule, as the oracle loop does."""
    data = proto["data"]
    eng = build_engine(data, cfg_for(3, 3, background=True,
                                     background_warmup=0), device="cpu")
    eng.run_em(3)
    ref = bo.em_fit(data, 3, 3, warmup=0)
    assert eng._bg_on and eng._bg_plain_iters == 0
    assert eng.background_pi == pytest.approx(ref["pi0"], rel=1e-4)
    # and a warm-up longer than the run leaves the fit plain
    eng = build_engine(data, cfg_for(3, 3, background=True,
                                     background_warmup=7), device="cpu")
    eng.run_em(3)
    assert not eng._bg_on and eng.background_pi == 0.0
    assert eng._bg_plain_iters == 3


def test_epsilon_loop_honours_switch_on(proto):
    cfg = GmmConfig(num_clusters=3, target_num_clusters=3, min_iters=8,
                    max_iters=30, background=True)
    eng = build_engine(proto["data"], cfg, device="cpu")
    eng.run_em(3)
    assert eng._bg_on
    assert abs(eng.background_pi - 600 / 6600) <= 0.005


# ----------------------------------------------------------------- weights
D3, K3 = 3, 3


@pytest.fixture(scope="module")
def small():
    data, labels = bo.blobs_plus_noise(5, d=D3, k=K3, per_blob=200,
                                       n_noise=60, scale=1.0, spread=20.0)
    s = np.random.default_rng(5).integers(0, 4, size=data.shape[0])
    return data, labels, s.astype(np.float32)


def collect(eng, k=K3):
    lik = eng.run_em(k)
    st = eng.state.shrink(k)
    return {"N": np.append(st.N.numpy().astype(np.float64),
                           eng.background_n),
            "pi0": np.array([eng.background_pi]),
            "means": (st.means + eng.center.unsqueeze(0)).numpy()
            .astype(np.float64),
            "R": st.R.numpy().astype(np.float64),
            "lik": np.array([lik])}


def reldiff(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def worst(a, b):
    return max(reldiff(a[q], b[q]) for q in a)


def direct_engine(rows, total, center, seeds, var, ln_v, weights=None):
    return EmEngine(torch.from_numpy(rows),
                    cfg_for(K3, 12, background=True, background_warmup=3),
                    total, center, seeds, var, device="cpu",
                    weights_shard=(None if weights is None
                                   else torch.from_numpy(weights)),
                    background_log_volume=ln_v)


@pytest.fixture(scope="module")
def replicated(small):
    """As in test_weights_cpu.py: the fit on the replicated rows, and the
    reordering floor measured as the difference to the same fit on a fixed
    permutation of them; the weighted comparisons allow 8x that floor."""
    data, labels, s = small
    rows = np.repeat(data, s.astype(np.int64), axis=0)
    total = int(s.sum())
    rt = torch.from_numpy(rows).double()
    center = rt.mean(dim=0).float()
    var = (rt.pow(2).mean(dim=0) - rt.mean(dim=0).pow(2)).float()
    seeds = torch.from_numpy(np.stack([
        data[np.nonzero((labels == c) & (s > 0))[0][0]] for c in range(K3)]))
    ln_v = bo.log_volume(data, s)
    ref = collect(direct_engine(rows, total, center, seeds, var, ln_v))
    perm = np.random.default_rng(99).permutation(total)
    ref_p = collect(direct_engine(np.ascontiguousarray(rows[perm]), total,
                                  center, seeds, var, ln_v))
    floor = worst(ref_p, ref)
    print(f"reordering floor: {floor:.3e}")
    assert floor > 0.0 and ref["pi0"][0] > 0.02
    return {"total": total, "center": center, "var": var, "seeds": seeds,
            "ln_v": ln_v, "ref": ref, "floor": floor}


def test_integer_weights_equal_replicated_rows(small, replicated):
    data, _, s = small
    r = replicated
    eng = direct_engine(data, r["total"], r["center"], r["seeds"], r["var"],
                        r["ln_v"], weights=s)
    got = collect(eng)
    for q in got:
        print(f"{q}: {reldiff(got[q], r['ref'][q]):.3e} "
              f"(floor {r['floor']:.3e})")
    assert worst(got, r["ref"]) <= 8.0 * r["floor"]


def test_mask_equals_subset(small, replicated):
    data, _, s = small
    mask = (s > 0).astype(np.float32)
    cfg = cfg_for(K3, 12, background=True, background_warmup=3)
    eng_w = build_engine(data, cfg, device="cpu", weights=mask)
    eng_s = build_engine(data[mask > 0], cfg, device="cpu")
    assert eng_w.bg_log_volume == eng_s.bg_log_volume
    got, ref = collect(eng_w), collect(eng_s)
    for q in got:
        print(f"{q}: {reldiff(got[q], ref[q]):.3e}")
    assert worst(got, ref) <= 8.0 * replicated["floor"]


def test_zero_weight_rows_get_posteriors_but_no_share(small):
    data, _, s = small
    cfg = cfg_for(K3, 12, background=True, background_warmup=3)
    eng = build_engine(data, cfg, device="cpu", weights=s)
    eng.run_em(K3)
    post = eng.posteriors(K3)
    assert post.shape == (K3 + 1, data.shape[0])
    assert float((post.sum(dim=0) - 1.0).abs().max()) <= 1e-5
    # far-out garbage in zero-weight rows: certain background events that
    # change neither the box nor n0 nor anything else
    garbage = data.copy()
    zero_rows = np.nonzero(s == 0)[0]
    garbage[zero_rows[:5]] = 4.0e3
    eng_g = build_engine(garbage, cfg, device="cpu", weights=s)
    eng_g.run_em(K3)
    assert eng_g.bg_log_volume == eng.bg_log_volume
    assert eng_g.background_n == eng.background_n
    assert eng_g.background_pi == eng.background_pi
    assert torch.equal(eng_g.state.N, eng.state.N)
    post_g = eng_g.posteriors(K3)
    assert bool((post_g[K3, zero_rows[:5]] == 1.0).all())
    w = eng.recompute_memberships(eng.state.shrink(K3))
    assert w.shape == (K3 + 1, data.shape[0])
    assert float((w - post).abs().max()) <= 1e-5


# --------------------------------------------------------- scores and sweep
def test_mdl_extra_parameter():
    base = rissanen_score(-1234.5, 7, 20, 6600)
    assert rissanen_score(-1234.5, 7, 20, 6600, extra_params=0) == base
    got = rissanen_score(-1234.5, 7, 20, 6600, extra_params=1)
    assert got - base == pytest.approx(0.5 * np.log(6600 * 20.0), rel=1e-12)


def test_sweep_keeps_noise_in_background(proto):
    cfg = GmmConfig(num_clusters=5, target_num_clusters=3, min_iters=20,
                    max_iters=20, background=True)
    eng = build_engine(proto["data"], cfg, device="cpu")
    res = eng.sweep()
    print(f"K {res.num_clusters}, pi0 {res.background_pi!r}, by K "
          f"{res.rissanen_by_k}")
    assert res.num_clusters == 3
    assert abs(res.background_pi - 600 / 6600) <= 0.01
    assert res.background_n == pytest.approx(res.background_pi * 6600,
                                             rel=1e-5)
    assert res.background_log_volume == eng.bg_log_volume
    # the score of a K counts the background's weight as a parameter
    assert res.min_rissanen == pytest.approx(rissanen_score(
        res.likelihood, 3, 20, 6600, extra_params=1))


# -------------------------------------------- config, model files, CLI
@pytest.mark.parametrize("kw", [
    {"background_init": 0.0}, {"background_init": 1.0},
    {"background_warmup": -1}, {"background_warmup": 2.5},
    {"background_log_volume": float("nan")},
    {"background": True, "checkpoint_dir": "/nonexistent"},
])
def test_config_validation(kw):
    with pytest.raises(ValueError):
        GmmConfig(num_clusters=2, **kw).validate()


def test_config_defaults():
    cfg = GmmConfig()
    assert (cfg.background, cfg.background_init, cfg.background_warmup,
            cfg.background_log_volume) == (False, 0.01, 5, None)
    GmmConfig(num_clusters=2, background=True,
              background_log_volume=-3.0).validate()


def test_engine_needs_a_volume(small):
    data = torch.from_numpy(small[0])
    cfg = cfg_for(K3, 2, background=True)
    with pytest.raises(ValueError, match="volume"):
        EmEngine(data, cfg, data.shape[0], data.mean(dim=0), data[:K3],
                 data.var(dim=0), device="cpu")
    from cuda_gmm_mpi_amd.engine import build_engine_sharded
    with pytest.raises(ValueError, match="scatter"):
        build_engine_sharded(data, cfg, data.shape[0], data.mean(dim=0),
                             data.var(dim=0), data[:K3])


def plain_model():
    rng = np.random.default_rng(8)
    means = rng.standard_normal((2, 3)).astype(np.float32) * 5
    r = np.stack([np.eye(3, dtype=np.float32) * (c + 1) for c in range(2)])
    return means, r, np.array([0.25, 0.75], np.float32)


def test_plain_model_file_is_version_1(tmp_path):
    means, r, pi = plain_model()
    model = GmmModel.from_params(means, r, pi)
    assert not model.has_background
    path = str(tmp_path / "m.npz")
    model.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(
            ["format_version", "center", "means_centered", "pi", "N",
             "constant", "avgvar", "R", "Rinv", "diag_only", "bug_compat"])
        assert float(z["format_version"]) == 1.0
        assert all(z[q].dtype == np.float32 for q in z.files)
    back = GmmModel.load(path)
    assert back.background_pi == 0.0 and back.background_log_volume == 0.0


def test_background_model_round_trip_and_strict_keys(tmp_path):
    means, r, pi = plain_model()
    model = GmmModel.from_params(means, r, pi, background_pi=0.125,
                                 background_log_volume=-7.5)
    path = str(tmp_path / "m2.npz")
    model.save(path)
    with np.load(path) as z:
        assert float(z["format_version"]) == 2.0
        fields = {q: z[q] for q in z.files}
    assert {"background_pi", "background_log_volume"} <= set(fields)
    back = GmmModel.load(path)
    assert back.background_pi == 0.125
    assert back.background_log_volume == -7.5
    assert torch.equal(back.pi, model.pi) and torch.equal(back.R, model.R)
    # version 2 keys under version 1, and version 2 without them
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, **{**fields, "format_version": np.float32(1)})
    with pytest.raises(ValueError, match="unexpected keys"):
        GmmModel.load(bad)
    fields.pop("background_pi")
    np.savez(bad, **fields)
    with pytest.raises(ValueError, match="missing keys"):
        GmmModel.load(bad)
    with pytest.raises(ValueError):
        GmmModel.from_params(means, r, pi, background_pi=1.0)


def test_predict_with_background(tmp_path):
    means, r, pi = plain_model()
    ln_v = 3 * np.log(200.0)
    model = GmmModel.from_params(means, r, pi, background_pi=0.1,
                                 background_log_volume=ln_v)
    plain = GmmModel.from_params(means, r, pi)
    rng = np.random.default_rng(2)
    data = np.concatenate([
        means[0] + rng.standard_normal((50, 3)),
        rng.uniform(-100, 100, (50, 3)),
        np.full((1, 3), 1.0e6)]).astype(np.float32)   # no cluster's number
    pred = model.predict(data, device="cpu")
    post = model.posteriors(data, device="cpu")
    assert post.shape == (3, 101)
    ok = np.isfinite(post).all(axis=0)
    assert ok[:100].all()
    assert np.abs(post[:, ok].sum(axis=0) - 1.0).max() <= 1e-5
    # -1 exactly where the background's posterior is strictly the largest
    want = np.where(post[2] > post[:2].max(axis=0), -1,
                    post[:2].argmax(axis=0))
    assert np.array_equal(pred.labels[ok], want[ok])
    assert pred.labels[100] == -1
    assert (pred.labels[:50] == 0).all() and (pred.labels[50:100] == -1).sum() >= 45
    np.testing.assert_allclose(pred.max_posterior[ok], post[:, ok].max(axis=0),
                               rtol=1e-5, atol=1e-7)
    assert pred.background_count == int((pred.labels == -1).sum())
    assert pred.counts.sum() + pred.background_count == 101
    # log_prob = ln((1 - pi0) p_gauss + pi0 / V)
    p_gauss = plain.predict(data, device="cpu").log_prob.astype(np.float64)
    ref = np.logaddexp(np.log(0.9) + p_gauss, np.log(0.1) - ln_v)
    np.testing.assert_allclose(pred.log_prob, ref, rtol=1e-5, atol=1e-5)
    assert plain.predict(data, device="cpu").background_count == 0


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory, small):
    from cuda_gmm_mpi_amd.cli import main
    tmp = tmp_path_factory.mktemp("bgcli")
    data = small[0]
    binpath = str(tmp / "d.bin")
    gio.write_bin(binpath, data)
    out = str(tmp / "o")
    model_path = str(tmp / "m.npz")
    metrics = str(tmp / "metrics.json")
    rc = main(["3", binpath, out, "3", "--background", "--background-warmup",
               "3", "--min-iters", "12", "--max-iters", "12", "--device",
               "cpu", "--save-model", model_path, "--metrics-out", metrics])
    assert rc == 0
    return {"tmp": tmp, "bin": binpath, "out": out, "model": model_path,
            "metrics": metrics, "data": data}


def test_cli_summary_results_and_metrics(cli_run, small):
    import json
    labels = small[1]
    n = cli_run["data"].shape[0]
    s = gio.read_summary(cli_run["out"] + ".summary")
    pi0 = float(s["background_pi"])
    truth = float((labels == -1).mean())
    print(f"pi0 {pi0} truth {truth}")
    assert abs(pi0 - truth) <= 0.03
    # the Probability lines are mixture weights: with the background's, 1
    assert float(s["pi"].astype(np.float64).sum()) + pi0 == pytest.approx(
        1.0, abs=5e-6)
    assert float(s["N"].astype(np.float64).sum()) + float(
        s["background_n"]) == pytest.approx(n, abs=1e-2)
    assert float(s["background_log_volume"]) == pytest.approx(
        bo.log_volume(cli_run["data"]), abs=1e-6)
    text = open(cli_run["out"] + ".summary").read()
    assert text.rstrip().splitlines()[-4] == "Background"
    lines = open(cli_run["out"] + ".results").read().splitlines()
    assert len(lines) == n
    rows = np.array([[float(v) for v in ln.split("\t")[1].split(",")]
                     for ln in lines])
    assert rows.shape == (n, 4)
    assert np.abs(rows.sum(axis=1) - 1.0).max() <= 1e-4
    assert (rows[labels == -1, 3] > 0.5).mean() >= 0.9
    m = json.load(open(cli_run["metrics"]))
    assert m["background_pi"] == pytest.approx(pi0, abs=1e-6)
    assert m["background_n"] == pytest.approx(pi0 * n, rel=1e-4)
    assert m["background_log_volume"] == pytest.approx(
        float(s["background_log_volume"]), abs=1e-6)


def test_cli_model_and_summary_round_trip(cli_run, small):
    from cuda_gmm_mpi_amd import classify
    labels = small[1]
    model = GmmModel.load(cli_run["model"])
    assert model.has_background
    with np.load(cli_run["model"]) as z:
        assert float(z["format_version"]) == 2.0
    s = gio.read_summary(cli_run["out"] + ".summary")
    assert model.background_pi == pytest.approx(float(s["background_pi"]),
                                                abs=1e-6)
    assert float(model.pi.sum()) == pytest.approx(1.0, abs=1e-5)
    lossy = GmmModel.from_summary(cli_run["out"] + ".summary")
    assert lossy.background_pi == float(s["background_pi"])
    assert lossy.background_log_volume == float(s["background_log_volume"])
    assert float(lossy.pi.sum()) == pytest.approx(1.0, abs=1e-5)
    np.testing.assert_allclose(lossy.pi.numpy(), model.pi.numpy(), atol=1e-5)
    # .labels of both: -1 for the noise
    for name, src in (("a", cli_run["model"]),
                      ("b", cli_run["out"] + ".summary")):
        stem = str(cli_run["tmp"] / name)
        assert classify.main([src, cli_run["bin"], stem, "--device", "cpu",
                              "--memberships"]) == 0
        lab = np.array([int(ln.split(",")[0])
                        for ln in open(stem + ".labels")])
        assert set(lab.tolist()) <= {-1, 0, 1, 2}
        assert (lab[labels == -1] == -1).mean() >= 0.9
        assert (lab[labels >= 0] == -1).mean() <= 0.02
        first = open(stem + ".results").readline()
        assert len(first.split("\t")[1].split(",")) == 4


def test_predict_reproduces_the_runs_memberships(small, tmp_path):
    from cuda_gmm_mpi_amd.cli import run_clustering
    data = small[0]
    cfg = cfg_for(K3, 12, background=True, background_warmup=3)
    cfg.enable_output = False
    res = run_clustering(data, cfg, str(tmp_path / "a"), "cpu",
                         write_results=False)
    mem = res["memberships"]
    assert mem.shape == (K3 + 1, data.shape[0])
    model = res["model"]
    assert model.background_pi == res["background_pi"] > 0.0
    post = model.posteriors(data, device="cpu")
    assert np.array_equal(post, mem)
    pred = model.predict(data, device="cpu")
    want = np.where(mem[K3] > mem[:K3].max(axis=0), -1,
                    mem[:K3].argmax(axis=0))
    # posteriors within rounding of a tie may fall either way
    top = np.sort(mem, axis=0)
    clear = top[-1] - top[-2] > 1e-5
    assert clear.mean() >= 0.99
    assert np.array_equal(pred.labels[clear], want[clear])
    assert pred.background_count == int((pred.labels == -1).sum())
    # without the flag the result carries no background
    cfg0 = cfg_for(K3, 4)
    cfg0.enable_output = False
    res0 = run_clustering(data, cfg0, str(tmp_path / "b"), "cpu",
                          write_results=False)
    assert res0["background_pi"] is None
    assert res0["memberships"].shape[0] == K3
    assert not res0["model"].has_background


def test_cli_refusals(tmp_path, small, capsys):
    from cuda_gmm_mpi_amd.cli import main
    binpath = str(tmp_path / "d.bin")
    gio.write_bin(binpath, small[0])
    out = str(tmp_path / "o")
    args = ["3", binpath, out, "3", "--background", "--min-iters", "2",
            "--max-iters", "2", "--device", "cpu"]
    assert main(args + ["--scatter-input"]) == 1
    assert "--scatter-input" in capsys.readouterr().out
    assert main(args + ["--checkpoint-dir", str(tmp_path / "ck")]) == 1
    assert "checkpoint" in capsys.readouterr().out
    assert main(args + ["--background-init", "1.5"]) == 1
    assert main(args + ["--background-warmup", "-2"]) == 1


# ------------------------------------------------------------ world 2, gloo
def _fit_background():
    data, _ = bo.blobs_plus_noise(2, d=3, k=3, per_blob=600, n_noise=202,
                                  scale=1.0, spread=20.0)   # 2002 rows
    # avgvar ~ 0: the G*avgvar regularization is world-size dependent by
    # design, as in test_dist_gloo.py
    cfg = GmmConfig(num_clusters=3, target_num_clusters=3, min_iters=8,
                    max_iters=8, covariance_dynamic_range=1e15,
                    background=True, background_warmup=3)
    eng = build_engine(data, cfg, device="cpu")
    lik = eng.run_em(3)
    w = eng.recompute_memberships(eng.state.shrink(3))
    gathered = eng.gather_memberships(w)
    return {"lik": lik, "pi0": eng.background_pi, "n0": eng.background_n,
            "ln_v": eng.bg_log_volume,
            "rows": None if gathered is None else gathered.shape,
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
        result = _fit_background()
        if rank == 0:
            out_q.put(result)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_background_matches_single_process():
    single = _fit_background()
    assert single["pi0"] > 0.05
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29841, q))
             for r in range(2)]
    for p in procs:
        p.start()
    multi = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert multi["ln_v"] == single["ln_v"]
    assert multi["rows"] == single["rows"] == (4, 2002)
    print(f"pi0 world 2 {multi['pi0']!r} world 1 {single['pi0']!r}")
    # the tolerances of test_dist_gloo's world-2 EM test (pi0 as pi)
    assert multi["pi0"] == pytest.approx(single["pi0"], rel=1e-3)
    assert multi["n0"] == pytest.approx(single["n0"], rel=1e-3)
    assert multi["lik"] == pytest.approx(single["lik"], rel=1e-4)
    np.testing.assert_allclose(multi["N"], single["N"], rtol=1e-3)
    np.testing.assert_allclose(multi["means"], single["means"],
                               rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(multi["R"], single["R"], rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(multi["pi"], single["pi"], rtol=1e-3)
