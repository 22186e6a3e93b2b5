"""Student-t mixture components on the CPU engine path: the float64 oracle
of student_t_oracle.py and its fp32 twins, the engine on the three-blob t3
dataset against the oracle's EM loop, weights, large nu, model files, the
command line and a gloo world of 2.

Everything printed before an assertion is the measured figure next to its
bound. Every test here runs code the feature adds (the config field, the
twins, the engine's t path, the model and file formats) and fails without
it.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import student_t_oracle as so

from cuda_gmm_mpi_amd.engine import EmEngine, build_engine
from cuda_gmm_mpi_amd.models.model import GmmModel
from cuda_gmm_mpi_amd.ops import cpu_reference as cpu
from cuda_gmm_mpi_amd.ops import functional as F
from cuda_gmm_mpi_amd.utils import io as gio
from cuda_gmm_mpi_amd.utils.config import GmmConfig

INF = float("inf")
U32 = 2.0 ** -24
K3 = 3
ITERS = 60


def cfg_for(k, iters, **kw):
    return GmmConfig(num_clusters=k, target_num_clusters=k,
                     min_iters=iters, max_iters=iters, **kw)


# ------------------------------------------------------------------ twins
def logw_case(k=5, n=257, seed=3):
    """fp32 (logw, add, s): logw = add_c - q/2 for q including 0, 1e6 and
    +inf, one event with every q = +inf and weights with zeros."""
    rng = np.random.default_rng(seed)
    add = rng.uniform(-30.0, -5.0, k).astype(np.float32)
    q = rng.chisquare(24, (k, n)) * rng.choice([0.2, 1.0, 30.0], (k, n))
    q[0, 0], q[1, 1], q[2 % k, 2] = 0.0, 1e6, INF
    q[:, n // 2] = INF
    logw = (add[:, None] - np.float32(0.5) * q.astype(np.float32))
    s = rng.choice(np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=n)
    s[n // 3] = 0.0
    return logw.astype(np.float32), add, s


def test_oracle_delta_and_gaussian_limit():
    # nu = 1, D = 1 is the Cauchy density: 1 / (pi (1 + x^2))
    x = 1.7
    ln_t = (-0.5 * np.log(2 * np.pi) + so.delta(1.0, 1)
            - np.log1p(x * x))
    assert ln_t == pytest.approx(-np.log(np.pi * (1 + x * x)), abs=1e-12)
    # delta -> 0 and (nu + D)/2 log1p(q / nu) -> q / 2 as nu grows
    assert abs(so.delta(1e7, 24)) <= 1e-4
    assert cpu.student_t_delta(4.0, 24) == so.delta(4.0, 24)
    res = so.student_t_lse(np.array([[-3.0], [-4.0]]), [-1.0, -2.0], 1e9, 2)
    assert np.allclose(res["q"], 4.0)
    assert np.allclose(res["lt"], [[-3.0], [-4.0]], atol=1e-6)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nu", [1.0, 4.0, 1e4])
def test_cpu_twins_agree_with_oracle(nu, weighted):
    d = 24
    logw, add, s = logw_case()
    ref = so.student_t_lse(logw, add, nu, d, s if weighted else None)
    out, lse_t, lse_m, n_c, lik = cpu.student_t_lse(
        torch.from_numpy(logw), torch.from_numpy(add), nu, d,
        torch.from_numpy(s) if weighted else None)
    # the fp32 twin against the float64 contract on the same fp32 inputs:
    # every term of lt carries a few u of |add + delta| + (nu + D)/2 log1p
    h = 0.5 * (nu + d)
    with np.errstate(invalid="ignore", over="ignore"):
        scale = np.abs(add[:, None] + so.delta(nu, d)) + h * np.log1p(
            ref["q"] / nu) + np.abs(ref["lnu"])
    for name, got, want in (("out", out, ref["out"]),
                            ("lse_t", lse_t, ref["lse_t"]),
                            ("lse_m", lse_m, ref["lse_m"])):
        got = got.numpy().astype(np.float64)
        fin = np.isfinite(want)
        assert np.array_equal(got[~fin], want[~fin]), name
        sc = scale if got.ndim == 2 else np.where(
            np.isfinite(scale), scale, 0.0).max(axis=0) + 8 + np.abs(
                np.log(np.maximum(s, 1e-30)))
        ratio = float((np.abs(got[fin] - want[fin])
                       / (16 * U32 * np.maximum(1.0, sc[fin]))).max())
        print(f"twin {name} nu={nu} w={weighted}: err/tol {ratio:.3f}")
        assert ratio <= 1.0
    assert float(lse_t[logw.shape[1] // 2]) == -INF
    # n_c and lik: sums of N terms, each within the lse band above
    assert not bool(torch.isnan(n_c).any())
    np.testing.assert_allclose(n_c.numpy(), ref["n_c"], rtol=2e-4, atol=1e-4)
    assert float(lik) == ref["lik"] == -INF     # a live event at -inf
    if weighted:
        lm, _ = cpu.event_weight_lse(lse_t, torch.from_numpy(s),
                                     torch.log(torch.from_numpy(s)))
        assert torch.equal(lm, lse_m)
        assert bool((lse_m[torch.from_numpy(s == 0)] == INF).all())
    else:
        assert torch.equal(lse_m, lse_t)
    # posterior mode: lt only, tau sums to one where it is a number
    lt, lse_p, tau = cpu.student_t_posteriors(
        torch.from_numpy(logw), torch.from_numpy(add), nu, d)
    assert torch.equal(lse_p, lse_t)
    ok = np.isfinite(ref["lse_t"])
    assert float((tau[:, ok].sum(dim=0) - 1).abs().max()) <= 1e-5
    refp = so.student_t_lse(logw, add, nu, d, train=False)
    fin = np.isfinite(refp["out"])
    assert np.array_equal(lt.numpy()[~fin], refp["out"][~fin])


@pytest.mark.parametrize("k", [1, 3, 64, 257])
def test_pi_twin_agrees_with_oracle(k):
    rng = np.random.default_rng(k)
    n_c = rng.uniform(1.0, 500.0, k).astype(np.float32)
    if k > 1:
        n_c[k // 2] = 0.25          # an emptied cluster: the 1e-10 floor
    const = rng.uniform(-40, -10, k).astype(np.float32)
    n, pi, add = cpu.student_t_pi(torch.from_numpy(n_c),
                                  torch.from_numpy(const))
    rn, rpi, radd = so.student_t_pi(n_c, const)
    assert np.array_equal(n.numpy(), n_c)
    np.testing.assert_allclose(pi.numpy(), rpi, rtol=(k + 4) * U32)
    np.testing.assert_allclose(add.numpy(), radd, rtol=8 * U32,
                               atol=(k + 4) * U32)
    if k > 1:
        assert float(pi[k // 2]) == np.float32(1e-10)
    # through functional, with and without the add buffer
    st_n, st_pi = torch.zeros(k), torch.zeros(k)
    F.student_t_pi(torch.from_numpy(n_c), None, st_n, st_pi)
    assert torch.equal(st_pi, pi) and torch.equal(st_n, n)


# ------------------------------------------------------ engine vs the oracle
@pytest.fixture(scope="module")
def blobs():
    data, labels = so.t3_blobs()
    return {"data": data, "labels": labels,
            "gauss": so.em_fit(data, K3, ITERS),
            "t4": so.em_fit(data, K3, ITERS, nu=4.0)}


def engine_trace(data, nu, iters=ITERS, weights=None):
    eng = build_engine(data, cfg_for(K3, 1, student_t_nu=nu), device="cpu",
                       weights=weights)
    liks = [eng._reduce_likelihood(eng._estep(K3))]
    for _ in range(iters):
        eng._mstep(K3)
        liks.append(eng._reduce_likelihood(eng._estep(K3)))
    return eng, np.array(liks)


@pytest.fixture(scope="module")
def engine_t4(blobs):
    return engine_trace(blobs["data"], 4.0)


def traces(r):
    return np.array([float(np.trace(np.asarray(m, dtype=np.float64)))
                     for m in r])


def test_likelihood_traces_monotone_and_engine_follows_oracle(blobs,
                                                              engine_t4):
    for name in ("gauss", "t4"):
        trace = blobs[name]["liks"]
        step = float(np.diff(trace).min())
        print(f"{name}: smallest likelihood step {step:.3e}, ln L "
              f"{trace[-1]:.3f}")
        # the slack of test_engine_cpu.py's monotone checks
        assert (np.diff(trace) > -abs(trace[-1]) * 1e-5).all()
    assert blobs["t4"]["lik"] > blobs["gauss"]["lik"] + 500.0
    _, liks = engine_t4
    ref = blobs["t4"]["liks"]
    rel = float(np.abs(liks - ref).max() / abs(ref[-1]))
    print(f"engine vs oracle likelihood trace: {rel:.3e} of |L| "
          f"(bound 1e-5); last {liks[-1]!r} vs {ref[-1]!r}")
    assert rel <= 1e-5
    assert (np.diff(liks) > -abs(liks[-1]) * 1e-5).all()


def test_fit_quality_scale_traces(blobs, engine_t4):
    eng, _ = engine_t4
    g = traces(blobs["gauss"]["R"])
    t = traces(eng.state.shrink(K3).R.numpy())
    print(f"scale-matrix traces (truth 4): gaussian {g.round(2)}, "
          f"t nu=4 {t.round(2)}, oracle t {traces(blobs['t4']['R']).round(2)}")
    assert (g > 8.0).all()
    assert (np.abs(t - 4.0) < np.abs(g - 4.0)).all()
    means = (eng.state.shrink(K3).means + eng.center.unsqueeze(0)).numpy()
    err_t = float(np.abs(means - so.T3_CENTRES).max())
    err_g = float(np.abs(blobs["gauss"]["means"] - so.T3_CENTRES).max())
    print(f"max mean error: t {err_t:.3f}, gaussian {err_g:.3f}")
    assert err_t < err_g
    # and the engine's fit is the oracle's
    np.testing.assert_allclose(eng.state.shrink(K3).R.numpy(),
                               blobs["t4"]["R"], rtol=1e-3, atol=1e-3)


def test_stationarity_sum_tau_u_over_sum_tau(blobs, engine_t4):
    """At a stationary point sum tau u = sum tau per cluster: the
    parameter-expanded M-step and the textbook one then coincide. After 60
    iterations the oracle is within 5e-5 (1.0000 to four places); the fp32
    engine gets twice that."""
    dev_o = float(np.abs(blobs["t4"]["ratio"] - 1.0).max())
    eng, _ = engine_t4
    tau = eng.posteriors(K3)
    ratio = (eng._w_s.sum(dim=1) / tau.sum(dim=1)).numpy()
    dev_e = float(np.abs(ratio - 1.0).max())
    print(f"|sum tau u / sum tau - 1|: oracle {dev_o:.3e} (bound 5e-5), "
          f"engine {dev_e:.3e} (bound 1e-4)")
    assert dev_o <= 5e-5 and dev_e <= 1e-4
    # N and pi are the responsibilities', not the moments' corner
    n = eng.state.shrink(K3).N
    assert float(n.sum()) == pytest.approx(1200.0, rel=1e-5)
    assert float(eng.state.shrink(K3).pi.sum()) == pytest.approx(1.0,
                                                                 abs=1e-5)
    assert float((tau.sum(dim=0) - 1.0).abs().max()) <= 1e-5


def test_large_nu_approaches_the_gaussian_fit(blobs):
    """nu = 1e4. The float64 oracle's own gap between the nu = 1e4 fit and
    the Gaussian fit here is 1.424 in ln L (1.4e-4 of |L|) and 0.0113 in the
    largest entry of R; the engine's gap may be three times that."""
    data = blobs["data"]
    big = so.em_fit(data, K3, ITERS, nu=1e4)
    gap_l = abs(big["lik"] - blobs["gauss"]["lik"])
    gap_r = float(np.abs(big["R"] - blobs["gauss"]["R"]).max())
    eng_t = build_engine(data, cfg_for(K3, ITERS, student_t_nu=1e4),
                         device="cpu")
    eng_g = build_engine(data, cfg_for(K3, ITERS), device="cpu")
    lik_t, lik_g = eng_t.run_em(K3), eng_g.run_em(K3)
    e_l = abs(lik_t - lik_g)
    e_r = float((eng_t.state.R - eng_g.state.R).abs().max())
    print(f"nu=1e4 vs gaussian: oracle gaps ln L {gap_l:.4f} R {gap_r:.5f}; "
          f"engine gaps ln L {e_l:.4f} R {e_r:.5f} (bounds 3x the oracle's)")
    assert 0.0 < gap_l <= 2.0 and gap_r <= 0.02
    assert e_l <= 3.0 * gap_l and e_r <= 3.0 * gap_r
    assert lik_t == pytest.approx(big["lik"], rel=1e-5)


def test_nu_zero_is_the_plain_fit_bit_for_bit(blobs):
    data = blobs["data"]
    eng_off = build_engine(data, cfg_for(K3, 8, student_t_nu=0.0),
                           device="cpu")
    eng_plain = build_engine(data, cfg_for(K3, 8), device="cpu")
    assert eng_off.run_em(K3) == eng_plain.run_em(K3)
    for eng in (eng_off, eng_plain):
        assert not eng.student_t and eng._t_n is None and eng._w_s is None
    for q in ("N", "pi", "means", "R", "constant"):
        assert torch.equal(getattr(eng_off.state, q),
                           getattr(eng_plain.state, q)), q
    assert torch.equal(eng_off.w, eng_plain.w)


# ----------------------------------------------------------------- weights
def collect(eng, k=K3):
    lik = eng.run_em(k)
    st = eng.state.shrink(k)
    return {"N": st.N.numpy().astype(np.float64),
            "means": (st.means + eng.center.unsqueeze(0)).numpy()
            .astype(np.float64),
            "R": st.R.numpy().astype(np.float64),
            "lik": np.array([lik])}


def reldiff(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def worst(a, b):
    return max(reldiff(a[q], b[q]) for q in a)


def direct_engine(rows, total, center, seeds, var, weights=None):
    return EmEngine(torch.from_numpy(rows),
                    cfg_for(K3, 12, student_t_nu=4.0), total, center, seeds,
                    var, device="cpu",
                    weights_shard=(None if weights is None
                                   else torch.from_numpy(weights)))


@pytest.fixture(scope="module")
def small():
    data, labels = so.t3_blobs(seed=7, per=150)
    s = np.random.default_rng(5).integers(0, 4, size=data.shape[0])
    return data, labels, s.astype(np.float32)


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
    ref = collect(direct_engine(rows, total, center, seeds, var))
    perm = np.random.default_rng(99).permutation(total)
    ref_p = collect(direct_engine(np.ascontiguousarray(rows[perm]), total,
                                  center, seeds, var))
    floor = worst(ref_p, ref)
    print(f"reordering floor: {floor:.3e}")
    assert floor > 0.0
    return {"total": total, "center": center, "var": var, "seeds": seeds,
            "ref": ref, "floor": floor}


def test_integer_weights_equal_replicated_rows(small, replicated):
    data, _, s = small
    r = replicated
    got = collect(direct_engine(data, r["total"], r["center"], r["seeds"],
                                r["var"], weights=s))
    for q in got:
        print(f"{q}: {reldiff(got[q], r['ref'][q]):.3e} "
              f"(floor {r['floor']:.3e})")
    assert worst(got, r["ref"]) <= 8.0 * r["floor"]


def test_mask_equals_subset(small, replicated):
    data, _, s = small
    mask = (s > 0).astype(np.float32)
    cfg = cfg_for(K3, 12, student_t_nu=4.0)
    got = collect(build_engine(data, cfg, device="cpu", weights=mask))
    ref = collect(build_engine(data[mask > 0], cfg, device="cpu"))
    for q in got:
        print(f"{q}: {reldiff(got[q], ref[q]):.3e}")
    assert worst(got, ref) <= 8.0 * replicated["floor"]


def test_weighted_engine_matches_weighted_oracle(small):
    data, _, s = small
    ref = so.em_fit(data, K3, 12, nu=4.0, s=s)
    eng = build_engine(data, cfg_for(K3, 12, student_t_nu=4.0),
                       device="cpu", weights=s)
    lik = eng.run_em(K3)
    print(f"weighted ln L engine {lik!r} oracle {ref['lik']!r}")
    assert lik == pytest.approx(ref["lik"], rel=1e-5)
    # zero-weight rows get posteriors, but no share of the fit
    post = eng.posteriors(K3)
    assert float((post.sum(dim=0) - 1.0).abs().max()) <= 1e-5
    assert bool((eng._w_s[:, torch.from_numpy(s == 0)] == 0).all())
    assert float(eng.state.N.sum()) == pytest.approx(float(s.sum()),
                                                     rel=1e-5)


# ------------------------------------------------------- config and models
@pytest.mark.parametrize("kw", [
    dict(student_t_nu=-1.0), dict(student_t_nu=INF),
    dict(student_t_nu=float("nan")),
    dict(student_t_nu=4.0, background=True),
    dict(student_t_nu=4.0, checkpoint_dir="/tmp/ck"),
])
def test_config_validation(kw):
    with pytest.raises(ValueError):
        GmmConfig(**kw).validate()


def test_config_default_is_off():
    cfg = GmmConfig()
    assert cfg.student_t_nu == 0.0
    cfg.validate()
    GmmConfig(student_t_nu=4).validate()


def plain_model():
    rng = np.random.default_rng(8)
    means = rng.standard_normal((2, 3)).astype(np.float32) * 5
    r = np.stack([np.eye(3, dtype=np.float32) * (c + 1) for c in range(2)])
    return means, r, np.array([0.25, 0.75], np.float32)


def test_model_versions(tmp_path):
    means, r, pi = plain_model()
    v1 = GmmModel.from_params(means, r, pi)
    v2 = GmmModel.from_params(means, r, pi, background_pi=0.125,
                              background_log_volume=-7.5)
    v3 = GmmModel.from_params(means, r, pi, student_t_nu=4.0)
    assert not v1.is_student_t and v3.is_student_t
    base = ["format_version", "center", "means_centered", "pi", "N",
            "constant", "avgvar", "R", "Rinv", "diag_only", "bug_compat"]
    want = {1: base, 2: base + ["background_pi", "background_log_volume"],
            3: base + ["student_t_nu"]}
    fields = {}
    for ver, model in ((1, v1), (2, v2), (3, v3)):
        path = str(tmp_path / f"m{ver}.npz")
        model.save(path)
        with np.load(path) as z:
            assert sorted(z.files) == sorted(want[ver])
            assert float(z["format_version"]) == float(ver)
            fields[ver] = {q: z[q] for q in z.files}
        back = GmmModel.load(path)
        assert back.student_t_nu == (4.0 if ver == 3 else 0.0)
        assert back.background_pi == (0.125 if ver == 2 else 0.0)
        assert torch.equal(back.R, model.R)
        assert torch.equal(back.constant, model.constant)
    # versions 1 and 2 hold what they held before the field existed: the
    # arrays of the t model are the plain model's, only the scalar is new
    for q in base[1:]:
        assert np.array_equal(fields[1][q], fields[3][q]), q
        assert fields[1][q].dtype == np.float32
    assert fields[3]["student_t_nu"].dtype == np.float64
    # the key set is strict per version
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, **{**fields[3], "format_version": np.float32(1)})
    with pytest.raises(ValueError, match="unexpected keys"):
        GmmModel.load(bad)
    np.savez(bad, **{**fields[1], "format_version": np.float32(3)})
    with pytest.raises(ValueError, match="missing keys"):
        GmmModel.load(bad)
    with pytest.raises(ValueError):
        GmmModel.from_params(means, r, pi, student_t_nu=-2.0)
    with pytest.raises(ValueError):
        GmmModel.from_params(means, r, pi, student_t_nu=4.0,
                             background_pi=0.1, background_log_volume=1.0)


def test_summary_student_t_block_round_trip_and_truncation(tmp_path):
    means, r, pi = plain_model()
    model = GmmModel.from_params(means, r, pi, student_t_nu=2.5)
    state = model._on(torch.device("cpu"))
    path = str(tmp_path / "s.summary")
    gio.write_summary(path, state, True, None, 2.5)
    assert float(gio.read_summary(path)["student_t_nu"]) == 2.5
    assert GmmModel.from_summary(path).student_t_nu == 2.5
    text = open(path).read()
    # cut inside the block, and a block without its number
    for bad in (text[:text.index("Degrees of freedom")],
                text.replace("Degrees of freedom: 2.5", "Degrees of freedom:")):
        open(path, "w").write(bad)
        with pytest.raises(ValueError):
            gio.read_summary(path)
    gio.write_summary(path, state, True, None, 0.0)
    assert "Student-t" not in open(path).read()


def test_predict_scores_t_densities():
    means, r, pi = plain_model()
    model = GmmModel.from_params(means, r, pi, student_t_nu=4.0)
    rng = np.random.default_rng(2)
    data = np.concatenate([means[0] + rng.standard_normal((50, 3)),
                           means[1] + 3 * rng.standard_normal((50, 3))]
                          ).astype(np.float32)
    pred = model.predict(data, device="cpu")
    post = model.posteriors(data, device="cpu")
    assert post.shape == (2, 100)
    assert np.abs(post.sum(axis=0) - 1.0).max() <= 1e-5
    # float64 t densities from the definition
    x = data.astype(np.float64)
    lt = np.empty((2, 100))
    for c in range(2):
        diff = x - means[c].astype(np.float64)
        cov = r[c].astype(np.float64)
        q = (diff * np.linalg.solve(cov, diff.T).T).sum(axis=1)
        lt[c] = (np.log(float(pi[c])) - 1.5 * np.log(2 * np.pi)
                 - 0.5 * np.linalg.slogdet(cov)[1] + so.delta(4.0, 3)
                 - 3.5 * np.log1p(q / 4.0))
    m = lt.max(axis=0)
    ref = m + np.log(np.exp(lt - m).sum(axis=0))
    np.testing.assert_allclose(pred.log_prob, ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(post, np.exp(lt - ref), atol=1e-5)
    assert np.array_equal(pred.labels, post.argmax(axis=0))
    np.testing.assert_allclose(pred.max_posterior, post.max(axis=0),
                               rtol=1e-6)
    assert model.score(data, device="cpu") == pytest.approx(ref.sum(),
                                                           rel=1e-5)
    # heavier tails than the Gaussian model of the same parameters
    gauss = GmmModel.from_params(means, r, pi)
    far = np.full((1, 3), 60.0, np.float32)
    assert (model.predict(far, device="cpu").log_prob[0]
            > gauss.predict(far, device="cpu").log_prob[0] + 100.0)


# --------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def cli_run(tmp_path_factory, blobs):
    from cuda_gmm_mpi_amd.cli import main
    tmp = tmp_path_factory.mktemp("tcli")
    data = blobs["data"]
    binpath = str(tmp / "d.bin")
    gio.write_bin(binpath, data)
    out, out0 = str(tmp / "o"), str(tmp / "plain")
    model_path = str(tmp / "m.npz")
    metrics = str(tmp / "metrics.json")
    common = ["--min-iters", "12", "--max-iters", "12", "--device", "cpu"]
    assert main(["3", binpath, out, "3", "--student-t", "4", "--save-model",
                 model_path, "--metrics-out", metrics] + common) == 0
    assert main(["3", binpath, out0, "3"] + common) == 0
    return {"tmp": tmp, "bin": binpath, "out": out, "plain": out0,
            "model": model_path, "metrics": metrics, "data": data}


def test_cli_writes_tau_memberships_and_the_summary_block(cli_run):
    n = cli_run["data"].shape[0]
    lines = open(cli_run["out"] + ".results").read().splitlines()
    assert len(lines) == n
    rows = np.array([[float(v) for v in ln.split("\t")[1].split(",")]
                     for ln in lines])
    assert rows.shape == (n, 3)
    dev = float(np.abs(rows.sum(axis=1) - 1.0).max())
    print(f"membership rows sum to 1 within {dev:.2e}")
    assert dev <= 1e-4            # tau, never tau * u (%f text: 3 x 5e-7)
    text = open(cli_run["out"] + ".summary").read()
    assert text.rstrip().splitlines()[-2:] == ["Student-t",
                                              "Degrees of freedom: 4.0"]
    s = gio.read_summary(cli_run["out"] + ".summary")
    assert float(s["student_t_nu"]) == 4.0
    assert float(s["N"].sum()) == pytest.approx(n, abs=0.01)
    assert float(s["pi"].sum()) == pytest.approx(1.0, abs=5e-6)
    # without the flag: no block, no key
    plain = open(cli_run["plain"] + ".summary").read()
    assert "Student-t" not in plain
    assert "student_t_nu" not in gio.read_summary(
        cli_run["plain"] + ".summary")
    m = json.load(open(cli_run["metrics"]))
    assert m["student_t_nu"] == 4.0
    # scale matrices near the truth, the Gaussian run's inflated
    tr_t = traces(s["R"])
    tr_g = traces(gio.read_summary(cli_run["plain"] + ".summary")["R"])
    print(f"summary traces: t {tr_t}, gaussian {tr_g}")
    assert (np.abs(tr_t - 4.0) < np.abs(tr_g - 4.0)).all()


def test_cli_model_and_summary_round_trip(cli_run):
    from cuda_gmm_mpi_amd import classify
    model = GmmModel.load(cli_run["model"])
    assert model.student_t_nu == 4.0
    with np.load(cli_run["model"]) as z:
        assert float(z["format_version"]) == 3.0
    lossy = GmmModel.from_summary(cli_run["out"] + ".summary")
    assert lossy.student_t_nu == 4.0
    labels = {}
    for name, src in (("a", cli_run["model"]),
                      ("b", cli_run["out"] + ".summary")):
        stem = str(cli_run["tmp"] / name)
        assert classify.main([src, cli_run["bin"], stem, "--device", "cpu",
                              "--memberships"]) == 0
        labels[name] = np.array([int(ln.split(",")[0])
                                 for ln in open(stem + ".labels")])
    truth = np.repeat(np.arange(3), 400)
    assert (labels["a"] == truth).mean() >= 0.97
    assert (labels["a"] == labels["b"]).mean() >= 0.99
    # the saved model reproduces the run's memberships
    post = model.posteriors(cli_run["data"], device="cpu")
    rows = np.array([[float(v) for v in ln.split("\t")[1].split(",")]
                     for ln in open(cli_run["out"] + ".results")])
    assert np.abs(post.T - rows).max() <= 1e-6


def test_cli_refusals_and_result_dict(tmp_path, blobs, capsys):
    from cuda_gmm_mpi_amd.cli import main, run_clustering
    binpath = str(tmp_path / "d.bin")
    gio.write_bin(binpath, blobs["data"][:300])
    out = str(tmp_path / "o")
    args = ["3", binpath, out, "3", "--student-t", "4", "--min-iters", "2",
            "--max-iters", "2", "--device", "cpu"]
    assert main(args + ["--background"]) == 1
    assert "background" in capsys.readouterr().out
    assert main(args + ["--checkpoint-dir", str(tmp_path / "ck")]) == 1
    assert "checkpoint" in capsys.readouterr().out
    assert main(args[:4] + ["--student-t", "-3"] + args[6:]) == 1
    # it combines with --diag-only, --seed-method kmeans++ and --save-model
    assert main(args + ["--diag-only", "--seed-method", "kmeans++", "--seed",
                        "3", "--save-model", str(tmp_path / "m.npz")]) == 0
    assert GmmModel.load(str(tmp_path / "m.npz")).student_t_nu == 4.0
    cfg = cfg_for(K3, 4, student_t_nu=4.0)
    cfg.enable_output = False
    res = run_clustering(blobs["data"], cfg, str(tmp_path / "a"), "cpu",
                         write_results=False)
    assert res["student_t_nu"] == 4.0 and res["model"].student_t_nu == 4.0
    mem = res["memberships"]
    assert np.array_equal(res["model"].posteriors(blobs["data"],
                                                  device="cpu"), mem)
    assert np.abs(mem.sum(axis=0) - 1.0).max() <= 1e-5


# ------------------------------------------------------------ world 2, gloo
def _fit_t():
    data, _ = so.t3_blobs(seed=2, per=667)       # 2001 rows: uneven shards
    # avgvar ~ 0: the G*avgvar regularization is world-size dependent by
    # design, as in test_dist_gloo.py
    cfg = GmmConfig(num_clusters=3, target_num_clusters=3, min_iters=8,
                    max_iters=8, covariance_dynamic_range=1e15,
                    student_t_nu=4.0)
    eng = build_engine(data, cfg, device="cpu")
    lik = eng.run_em(3)
    w = eng.recompute_memberships(eng.state.shrink(3))
    gathered = eng.gather_memberships(w)
    return {"lik": lik,
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
        result = _fit_t()
        if rank == 0:
            out_q.put(result)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_matches_single_process():
    single = _fit_t()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29843, q))
             for r in range(2)]
    for p in procs:
        p.start()
    multi = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert multi["rows"] == single["rows"] == (3, 2001)
    print(f"N world 2 {multi['N']} world 1 {single['N']}")
    # the tolerances of test_dist_gloo's world-2 EM test
    assert multi["lik"] == pytest.approx(single["lik"], rel=1e-4)
    np.testing.assert_allclose(multi["N"], single["N"], rtol=1e-3)
    np.testing.assert_allclose(multi["means"], single["means"],
                               rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(multi["R"], single["R"], rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(multi["pi"], single["pi"], rtol=1e-3)
    # N sums to the event count on every world: the K-float all-reduce ran
    assert float(multi["N"].sum()) == pytest.approx(2001.0, rel=1e-5)
