"""Uniform background component on the GPU: background_lse and
background_update against the float64 oracle of background_oracle.py, the
engine on every E-step / M-step path against the CPU engine, graph replay
against eager launches, and predict on cuda against cpu. Every check prints
its figure next to the bound before it asserts."""
import numpy as np
import pytest
import torch

import background_oracle as bo

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.engine import build_engine  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402
from cuda_gmm_mpi_amd.utils.config import GmmConfig  # noqa: E402

INF = float("inf")
U32 = 2.0 ** -24   # fp32 unit roundoff
DEV = "cuda"

SIZES = [1, 63, 1024, 4097, 8195]


def kernel_case(n, seed=0):
    rng = np.random.default_rng([11, n, seed])
    lse = (rng.standard_normal(n) * 20 - 30).astype(np.float32)
    s = rng.choice(np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=n)
    if n >= 8:
        lse[n // 2] = -INF          # with whatever weight it drew
        lse[n // 3] = -INF
        s[n // 3] = 0.0             # and one with weight 0
    return lse, s


def b_values(lse):
    fin = lse[np.isfinite(lse)]
    top = float(fin.max()) if fin.size else 0.0
    # fp32 values: the kernel reads b from an fp32 device scalar
    return {"off": -INF, "inside": -35.0,
            "above": float(np.float32(top + 200.0))}


def bg_state(b):
    return torch.tensor([0.5, b, 0.0, 0.0], dtype=torch.float32, device=DEV)


def run_kernel(lse_t, b, s_t=None, lik=True, want_b=True):
    """One launch at the extension on NaN-prefilled outputs ->
    (lse_m, lse_b, n0 partials, likelihood partials or None)."""
    ext = hip_ext()
    n = lse_t.numel()
    before = lse_t.clone()
    empty = lse_t.new_empty(0)
    blocks = int(ext.event_weight_lse_blocks(n))
    nan = float("nan")
    lse_m = torch.full((n,), nan, device=DEV)
    lse_b = torch.full((n,), nan, device=DEV) if want_b else empty
    part = torch.full(((2 if lik else 1) * blocks,), nan, device=DEV)
    ext.background_lse(lse_t, bg_state(b),
                       s_t if s_t is not None else empty,
                       torch.log(s_t) if s_t is not None else empty,
                       lse_m, lse_b, part)
    torch.cuda.synchronize()
    assert torch.equal(lse_t, before), "lse was modified"
    assert not bool(torch.isnan(part).any()), "an unwritten partial slot"
    return (lse_m.cpu(), lse_b.cpu() if want_b else None,
            part[:blocks].cpu().numpy().astype(np.float64),
            part[blocks:].cpu().numpy().astype(np.float64) if lik else None)


def adds_per_thread(n):
    """fp32 additions into one thread's accumulator: 4 per vector it takes
    (one per 1024 events and block, grid capped at 2048) plus a tail
    event."""
    blocks = max(1, min((n + 1023) // 1024, 2048))
    return 4 * -(-(n // 4) // (256 * blocks)) + 1


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_background_lse_vs_oracle(n, weighted):
    lse, s = kernel_case(n)
    lse_t = torch.from_numpy(lse).to(DEV)
    s_t = torch.from_numpy(s).to(DEV) if weighted else None
    for name, b in b_values(lse).items():
        ref_b, ref_m, ref_n0, ref_lik = bo.background_lse(
            lse, b, s if weighted else None)
        got_m, got_b, n0_part, lik_part = run_kernel(lse_t, b, s_t)
        # ---- lse_b, lse_m: within 4 u max(1, |value|) of the oracle
        # rounded to fp32 (infinities exactly)
        for label, got, ref in (("lse_b", got_b, ref_b),
                                ("lse_m", got_m, ref_m)):
            got = got.numpy().astype(np.float64)
            ref32 = ref.astype(np.float32).astype(np.float64)
            fin = np.isfinite(ref32)
            assert np.array_equal(got[~fin], ref32[~fin]), (label, name)
            if fin.any():
                tol = 4 * U32 * np.maximum(1.0, np.abs(ref32[fin]))
                ratio = float((np.abs(got[fin] - ref32[fin]) / tol).max())
                print(f"BG {label} n={n} w={weighted} b={name} "
                      f"err/tol {ratio:.3f}")
                assert ratio <= 1.0, (label, name, ratio)
        # ---- exact cases
        lb = got_b.numpy()
        if weighted:
            # bitwise event_weight_lse of the kernel's own lse_b
            ew = torch.empty(n, device=DEV)
            F.event_weight_lse(got_b.to(DEV), s_t, torch.log(s_t), ew, False)
            assert torch.equal(ew.cpu(), got_m), name
            assert bool((got_m[torch.from_numpy(s == 0)] == INF).all())
        else:
            assert torch.equal(got_m, got_b), name
        if b == -INF:
            assert np.array_equal(lb, lse), "b = -inf must be the identity"
            assert (n0_part == 0.0).all()
        # ---- partials: the estep_lse rule of test_gpu_bigd_oracle.py,
        # (adds per thread + 10) u sum |terms|, on the kernel's own lse_b.
        # n0's terms s r0 come from r0 = expf(fl(b - lse_b)): the rounded
        # difference moves r0 by at most |t| e^-|t| u <= 0.37 u and expf by
        # an ulp or two of r0, so each term gets s (0.5 + 3 r0) u on top.
        live = (s > 0) if weighted else np.ones(n, bool)
        sw = s.astype(np.float64) if weighted else np.ones(n)
        lb64 = lb.astype(np.float64)
        adds = adds_per_thread(n) + (1 if weighted else 0)
        with np.errstate(invalid="ignore"):
            r0 = np.exp(b - lb64) if b != -INF else np.zeros(n)
        r0 = np.where(np.isnan(r0), 0.0, r0)
        n0_terms = sw[live] * r0[live]
        bound = U32 * ((adds + 10) * n0_terms.sum()
                       + (sw[live] * (0.5 + 3 * r0[live])).sum())
        diff = abs(n0_part.sum() - n0_terms.sum())
        print(f"BG n0 n={n} w={weighted} b={name} got {n0_part.sum()!r} "
              f"want {n0_terms.sum()!r} err/tol "
              f"{diff / bound if bound else 0.0:.3f}")
        assert diff <= bound
        # ... and against the oracle's own n0 with lse_b's tolerance folded
        # in: d r0 <= r0 * 4 u max(1, |lse_b|)
        fin = np.isfinite(lb64) & live
        slack = (sw[fin] * r0[fin] * 4 * U32
                 * np.maximum(1.0, np.abs(lb64[fin]))).sum()
        assert abs(n0_part.sum() - ref_n0) <= bound + slack
        lik_terms = sw[live] * lb64[live]
        if np.isfinite(lik_terms).all():
            bound = U32 * (adds + 10) * np.abs(lik_terms).sum()
            diff = abs(lik_part.sum() - lik_terms.sum())
            print(f"BG lik n={n} w={weighted} b={name} err/tol "
                  f"{diff / bound if bound else 0.0:.3f}")
            assert diff <= bound
        else:   # a live event at -inf: the sum is -inf, as unweighted EM's
            assert lik_part.sum() == lik_terms.sum() == -INF


@pytest.mark.parametrize("weighted", [False, True])
def test_background_lse_unaligned_views(weighted):
    """Views offset by one element take the scalar loop: bitwise the
    aligned result, partials included."""
    n = 4097
    lse, s = kernel_case(n + 1)
    lse_t = torch.from_numpy(lse).to(DEV)
    s_t = torch.from_numpy(s).to(DEV)
    b = -35.0
    view = run_kernel(lse_t[1:], b, s_t[1:] if weighted else None)
    alig = run_kernel(lse_t[1:].clone(), b,
                      s_t[1:].clone() if weighted else None)
    assert torch.equal(view[0], alig[0]) and torch.equal(view[1], alig[1])
    # the scalar loop gives a thread other events than the vector loop:
    # the sums agree to the summation bound, not bitwise
    lb64 = alig[1].numpy().astype(np.float64)
    sw = s[1:].astype(np.float64) if weighted else np.ones(n)
    live = sw > 0
    bound = U32 * (adds_per_thread(n) + 11) * np.abs(sw[live]
                                                     * lb64[live]).sum()
    assert abs(view[3].sum() - alig[3].sum()) <= 2 * bound
    assert abs(view[2].sum() - alig[2].sum()) <= 2 * U32 * 30 * max(
        alig[2].sum(), 1.0)
    # the outputs may be the unaligned ones, too
    ext = hip_ext()
    blocks = int(ext.event_weight_lse_blocks(n))
    out = torch.full((n + 1,), float("nan"), device=DEV)
    empty = out.new_empty(0)
    ext.background_lse(lse_t[1:].clone(), bg_state(b),
                       s_t[1:].clone() if weighted else empty,
                       torch.log(s_t[1:]).clone() if weighted else empty,
                       out[1:], empty, torch.empty(blocks, device=DEV))
    assert torch.equal(out[1:].cpu(), alig[0])
    assert bool(torch.isnan(out[0]))


def test_background_lse_likelihood_off_deterministic_and_checks():
    n = 8195
    lse, s = kernel_case(n, 1)
    lse_t = torch.from_numpy(lse).to(DEV)
    s_t = torch.from_numpy(s).to(DEV)
    on = run_kernel(lse_t, -35.0, s_t)
    off = run_kernel(lse_t, -35.0, s_t, lik=False, want_b=False)
    assert torch.equal(on[0], off[0])
    assert np.array_equal(on[2], off[2]) and off[3] is None
    again = run_kernel(lse_t, -35.0, s_t)
    assert torch.equal(on[0], again[0]) and torch.equal(on[1], again[1])
    assert np.array_equal(on[2], again[2])
    assert np.array_equal(on[3], again[3])
    # through functional: the likelihood lands in lik_out, or nowhere
    part = F.background_partial(n, DEV)
    assert part.shape == (2, 9)
    sentinel = torch.full((1,), -4242.0, device=DEV)
    lse_m = torch.empty(n, device=DEV)
    assert F.background_lse(lse_t, bg_state(-35.0), s_t, torch.log(s_t),
                            lse_m, part, need_lik=False,
                            lik_out=sentinel) is None
    assert float(sentinel.item()) == -4242.0
    lik = F.background_lse(lse_t, bg_state(-35.0), s_t, torch.log(s_t),
                           lse_m, part, lik_out=sentinel)
    assert lik.data_ptr() == sentinel.data_ptr()
    assert float(lik.item()) == pytest.approx(on[3].sum(), rel=1e-6)
    assert torch.equal(lse_m.cpu(), on[0])
    # argument checks happen before the launch
    ext = hip_ext()
    empty = lse_t.new_empty(0)
    good = torch.empty(9, device=DEV)
    with pytest.raises(RuntimeError):   # partial of another size
        ext.background_lse(lse_t, bg_state(0.0), empty, empty, lse_m, empty,
                           torch.empty(10, device=DEV))
    with pytest.raises(RuntimeError):   # short output
        ext.background_lse(lse_t, bg_state(0.0), empty, empty, lse_m[:-1],
                           empty, good)
    with pytest.raises(RuntimeError):   # s without lns
        ext.background_lse(lse_t, bg_state(0.0), s_t, empty, lse_m, empty,
                           good)
    with pytest.raises(RuntimeError):   # not the 4-float state
        ext.background_lse(lse_t, torch.zeros(2, device=DEV), empty, empty,
                           lse_m, empty, good)


@pytest.mark.parametrize("nparts", [1, 5, 300, 2048])
def test_background_update_vs_oracle(nparts):
    rng = np.random.default_rng(nparts)
    part = rng.uniform(0.0, 3.0, nparts).astype(np.float32)
    n_total, ln_v = 3.0 * nparts * 4.0, 41.5
    bg = F.background_state(DEV)
    assert bg.cpu().tolist() == [0.0, -INF, 0.0, 0.0]
    F.background_update(torch.from_numpy(part).to(DEV), n_total, ln_v, bg)
    got = bg.cpu().numpy().astype(np.float64)
    n0 = float(part.astype(np.float64).sum())
    pi0, b, add = bo.background_update(n0, n_total, ln_v)
    # n0 is an fp32 sum of nparts terms (<= nparts/256 + 10 additions per
    # path); pi0, b and lik_add follow it and are rounded once
    rel = (nparts / 256 + 12) * U32
    print(f"BG update nparts={nparts}: {got.tolist()} vs "
          f"{[pi0, b, add, n0]}")
    assert abs(got[3] - n0) <= rel * n0
    assert abs(got[0] - pi0) <= rel * pi0
    assert abs(got[1] - b) <= rel / (1 - pi0) + U32 * abs(b)
    assert abs(got[2] - add) <= (rel * pi0 / (1 - pi0) * n_total
                                 + U32 * abs(add))


def test_background_update_fixed_point_and_clamp():
    bg = bg_state(3.0)
    F.background_update(torch.zeros(7, device=DEV), 100.0, 5.0, bg)
    assert bg.cpu().tolist() == [0.0, -INF, 0.0, 0.0]
    F.background_update(torch.full((4,), 50.0, device=DEV), 100.0, 5.0, bg)
    pi0, b, add = bo.background_update(200.0, 100.0, 5.0)
    assert pi0 == 1.0 - 1e-6
    got = bg.cpu().numpy()
    assert got[0] == np.float32(pi0) and got[3] == 200.0
    assert got[1] == np.float32(b) and got[2] == np.float32(add)
    ext = hip_ext()
    with pytest.raises(RuntimeError):
        ext.background_update(torch.zeros(4, device=DEV), 5, 100.0, 5.0, bg)
    with pytest.raises(RuntimeError):
        ext.background_update(torch.zeros(4, device=DEV), 4, 0.0, 5.0, bg)


# ----------------------------------------------------------------- engine
def cfg_for(k, iters, **kw):
    return GmmConfig(num_clusters=k, target_num_clusters=k,
                     min_iters=iters, max_iters=iters, **kw)


def bg_cfg(k=3, iters=12, **kw):
    return cfg_for(k, iters, background=True, background_warmup=3, **kw)


def params(eng, k):
    st = eng.state.shrink(k)
    return {q: getattr(st, q).detach().cpu().clone()
            for q in ("N", "means", "R", "pi")}


_cases = {}


def engine_case(d, diag=False, weighted=False):
    """Blobs plus 10 % noise (N = 3000, K = 3), weights in {0, 0.5, 1, 2.5}
    when asked, and the CPU fit, computed once per shape. With weights the
    seed rows stride over the events with s > 0, so the arrangement (one
    seed per blob) is redone for those."""
    key = (d, diag, weighted)
    if key not in _cases:
        data, labels = bo.blobs_plus_noise(
            20 + d, d=d, k=3, per_blob=900, n_noise=300, scale=1.0,
            spread=12.0, mix=0.5 / np.sqrt(d))
        s = None
        if weighted:
            s = np.random.default_rng(d).choice(
                np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=len(data))
            keep = np.nonzero(s > 0)[0]
            seeds = [int(keep[p]) for p in bo.seed_rows(len(keep), 3)]
            for c, p in enumerate(seeds):
                if labels[p] == c:
                    continue
                q = next(int(j) for j in keep
                         if labels[j] == c and int(j) not in seeds)
                data[[p, q]] = data[[q, p]]
                labels[[p, q]] = labels[[q, p]]
        eng = build_engine(data, bg_cfg(diag_only=diag), device="cpu",
                           weights=s)
        lik = eng.run_em(3)
        assert eng.background_pi > 0.05
        _cases[key] = (data, s, params(eng, 3), eng.background_pi, lik)
    return _cases[key]


def check_engine(path, d, dtype, weighted):
    diag = path == "diag"
    data, s, ref, pi0_c, lik_c = engine_case(d, diag, weighted)
    eng = build_engine(data, bg_cfg(estep_dtype=dtype, diag_only=diag),
                       device=DEV, weights=s)
    if path == "valu":
        eng.use_fused_estep = False
        eng.mfac32 = None
    assert not eng.use_lds_estep
    assert eng.use_fused_estep == (path in ("fused", "diag"))
    assert eng.use_big_estep == (path == "big")
    lik_g = eng.run_em(3)
    assert eng._bg_on and eng._graphs and all(eng._graphs.values())
    got = params(eng, 3)
    pi0_g = eng.background_pi
    print(f"BG engine {path}/{dtype} w={weighted}: pi0 gpu {pi0_g!r} cpu "
          f"{pi0_c!r}; lik gpu {lik_g!r} cpu {lik_c!r}; max dN "
          f"{float((got['N'] - ref['N']).abs().max()):.3e}")
    assert abs(pi0_g - pi0_c) <= 1e-3
    # the tolerances of test_gpu_weights.py::test_weighted_em_gpu_matches_cpu
    np.testing.assert_allclose(got["N"].numpy(), ref["N"].numpy(), rtol=1e-3)
    np.testing.assert_allclose(got["means"].numpy(), ref["means"].numpy(),
                               rtol=1e-2, atol=1e-2)
    np.testing.assert_allclose(got["R"].numpy(), ref["R"].numpy(),
                               rtol=5e-2, atol=5e-2)
    post = eng.posteriors(3)
    assert post.shape == (4, data.shape[0])
    assert float((post.sum(dim=0) - 1.0).abs().max()) <= 1e-4
    mem = eng.recompute_memberships(eng.state.shrink(3))
    assert mem.shape == (4, data.shape[0])
    return eng


@pytest.mark.parametrize("path,d,dtype", [
    ("fused", 5, "bf16"), ("fused", 5, "fp32"),
    ("big", 40, "bf16"), ("big", 40, "fp32"),
    ("valu", 5, "fp32"), ("diag", 5, "fp32"),
])
def test_background_em_gpu_matches_cpu(path, d, dtype):
    check_engine(path, d, dtype, weighted=False)


@pytest.mark.parametrize("path,d,dtype", [("fused", 5, "bf16"),
                                          ("big", 40, "fp32")])
def test_background_weighted_em_gpu_matches_cpu(path, d, dtype):
    eng = check_engine(path, d, dtype, weighted=True)
    # a weighted fit keeps lse_b next to the shifted lse the moments read
    assert eng._lse_b.data_ptr() != eng._lse_w.data_ptr()
    assert bool((eng._lse_w[eng.s == 0] == INF).all())


def run_fit(data, cfg):
    eng = build_engine(data, cfg, device=DEV)
    lik = eng.run_em(cfg.num_clusters)
    torch.cuda.synchronize()
    return eng, lik


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_graph_replay_bitwise_equals_eager(monkeypatch, dtype):
    """12 iterations, warm-up 3: the switch-on (a device write and one
    launch between replays) falls inside the replayed range."""
    data = engine_case(5)[0]
    cfg = bg_cfg(estep_dtype=dtype)
    monkeypatch.delenv("GMM_NO_GRAPHS", raising=False)
    eng_g, lik_g = run_fit(data, cfg)
    assert eng_g._graphs and all(eng_g._graphs.values())
    monkeypatch.setenv("GMM_NO_GRAPHS", "1")
    eng_e, lik_e = run_fit(data, cfg)
    assert not eng_e._graphs
    print(f"BG graphs {dtype}: pi0 {eng_g.background_pi!r} / "
          f"{eng_e.background_pi!r}, lik {lik_g!r} / {lik_e!r}")
    assert torch.equal(eng_g._bg, eng_e._bg)
    assert lik_g == lik_e
    a, b = params(eng_g, 3), params(eng_e, 3)
    for q in a:
        assert torch.equal(a[q], b[q]), q
    assert torch.equal(eng_g._lse_w, eng_e._lse_w)


def test_background_off_is_the_plain_fit(monkeypatch):
    """background=False allocates and dispatches nothing: bitwise the fit
    of a config that never heard of the field."""
    monkeypatch.delenv("GMM_NO_GRAPHS", raising=False)
    data = engine_case(5)[0]
    eng_off, lik_off = run_fit(data, cfg_for(3, 12, background=False,
                                             estep_dtype="bf16"))
    eng_plain, lik_plain = run_fit(data, cfg_for(3, 12, estep_dtype="bf16"))
    for eng in (eng_off, eng_plain):
        assert eng._bg is None and eng._bg_partial is None
        assert eng._lse_b is None and eng._lse_w is None
        assert eng.use_lds_estep        # the default small-K path is kept
        assert eng.background_pi == 0.0
        assert eng.posteriors(3).shape == (3, data.shape[0])
    assert lik_off == lik_plain
    a, b = params(eng_off, 3), params(eng_plain, 3)
    for q in a:
        assert torch.equal(a[q], b[q]), q
    assert torch.equal(eng_off.w, eng_plain.w)


# ---------------------------------------------------------------- predict
@pytest.fixture(scope="module")
def trained():
    """D = 8, K = 3, N = 3000 with 10 % noise, fitted on the CPU."""
    from cuda_gmm_mpi_amd.models.model import GmmModel
    data, _ = bo.blobs_plus_noise(3, d=8, k=3, per_blob=900, n_noise=300,
                                  scale=1.0, spread=12.0,
                                  mix=0.5 / np.sqrt(8.0))
    eng = build_engine(data, bg_cfg(), device="cpu")
    eng.run_em(3)
    model = GmmModel.from_state(
        eng.state.shrink(3).clone(with_memberships=False), eng.center,
        background_pi=eng.background_pi,
        background_log_volume=eng.bg_log_volume)
    assert model.has_background
    return data, model


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_cuda_matches_cpu(trained, dtype):
    # the log_prob bands of test_gpu_classify.py
    bands = {"bf16": dict(rtol=5e-2, atol=2e-2),
             "fp32": dict(rtol=2e-3, atol=2e-4)}
    data, model = trained
    ref = model.predict(data, device="cpu")
    got = model.predict(data, device=DEV, estep_dtype=dtype)
    assert ref.background_count >= 250
    top = np.sort(model.posteriors(data, device="cpu"), axis=0)
    assert top.shape == (4, 3000)
    clear = top[-1] - top[-2] > 1e-3
    share = 1.0 - clear.mean()
    print(f"BG predict {dtype}: {100 * share:.3f} % within 1e-3 of a tie; "
          f"background {got.background_count} / {ref.background_count}")
    assert share <= 0.005
    assert np.array_equal(got.labels[clear], ref.labels[clear])
    assert (got.labels == -1).sum() == got.background_count
    np.testing.assert_allclose(got.log_prob, ref.log_prob, **bands[dtype])
    assert got.background_count == ref.background_count
    assert got.counts.sum() + got.background_count == 3000
    post = model.posteriors(data[:500], device=DEV, estep_dtype=dtype)
    assert post.shape == (4, 500)
    assert np.abs(post.sum(axis=0) - 1.0).max() <= 1e-4
