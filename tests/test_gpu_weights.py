"""Per-event training weights on the GPU: the event-weight kernel alone,
and weighted EM on every E-step/M-step path against the weighted CPU engine.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.engine import build_engine  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.utils.config import GmmConfig  # noqa: E402
from cuda_gmm_mpi_amd.utils.synthetic import make_supported_blobs  # noqa: E402

INF = float("inf")
U32 = 2.0 ** -24   # fp32 unit roundoff


def lik_bound(n, terms64):
    """Any-order fp32 summation of n terms plus one rounding per product:
    (n + 1) * 2^-24 * sum |s * lse|."""
    return (n + 1) * U32 * float(np.abs(terms64).sum())


def kernel_case(n, seed):
    rng = np.random.default_rng(seed)
    lse = (rng.standard_normal(n) * 20 - 30).astype(np.float32)
    s = rng.choice(np.array([0.0, 0.5, 1.0, 2.5, 3.7], np.float32), size=n)
    # one zero-weight event whose lse is -inf (n == 1: that is the event)
    z = n // 2
    s[z] = 0.0
    lse[z] = -INF
    return lse, s


def run_kernel(lse, s, need_lik=True, lik_out=None):
    lse_t = torch.from_numpy(lse).cuda()
    s_t = torch.from_numpy(s).cuda()
    lns_t = torch.log(s_t)
    out = torch.full_like(lse_t, 123.0)
    lik = F.event_weight_lse(lse_t, s_t, lns_t, out, need_lik,
                             lik_out=lik_out)
    torch.cuda.synchronize()
    assert torch.equal(lse_t.cpu(), torch.from_numpy(lse)), "lse was touched"
    return out.cpu(), lns_t.cpu(), lik


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1027, 4099])
def test_event_weight_kernel(n):
    cases = [kernel_case(n, 100 + n)]
    if n == 1:   # the single event with weight, too
        cases.append((np.array([-7.25], np.float32),
                      np.array([3.7], np.float32)))
    for lse, s in cases:
        out, lns, lik = run_kernel(lse, s)
        zero = s == 0
        want = torch.from_numpy(lse) - lns          # one fp32 subtraction
        want[torch.from_numpy(zero)] = INF
        assert torch.equal(out, want)
        assert bool((out[torch.from_numpy(zero)] == INF).all())
        terms = s[~zero].astype(np.float64) * lse[~zero].astype(np.float64)
        got = float(lik.item())
        bound = lik_bound(n, terms)
        print(f"n={n}: lik {got!r} vs {terms.sum()!r}, bound {bound:.3e}")
        assert abs(got - terms.sum()) <= bound
        _, _, lik2 = run_kernel(lse, s)
        assert lik2.item() == lik.item()              # deterministic


def test_event_weight_kernel_likelihood_off():
    lse, s = kernel_case(1027, 7)
    sentinel = torch.full((1,), -4242.0, device="cuda")
    out_on, _, _ = run_kernel(lse, s)
    out_off, _, lik = run_kernel(lse, s, need_lik=False, lik_out=sentinel)
    assert lik is None
    assert float(sentinel.item()) == -4242.0          # nothing was reduced
    assert torch.equal(out_on, out_off)
    # at the extension: an empty partial is the off switch, a wrong-sized
    # one is refused before launch, and a right-sized one is fully written
    from cuda_gmm_mpi_amd.ops.backend import hip_ext
    ext = hip_ext()
    lse_t = torch.from_numpy(lse).cuda()
    s_t = torch.from_numpy(s).cuda()
    out = torch.empty_like(lse_t)
    nblk = ext.event_weight_lse_blocks(lse_t.numel())
    assert nblk == 2
    with pytest.raises(RuntimeError):
        ext.event_weight_lse(lse_t, s_t, torch.log(s_t), out,
                             torch.empty(nblk + 1, device="cuda"))
    partial = torch.full((nblk,), float("nan"), device="cuda")
    ext.event_weight_lse(lse_t, s_t, torch.log(s_t), out, partial)
    assert bool(torch.isfinite(partial).all())


def test_event_weight_kernel_unaligned_views():
    """Views that are not 16-byte aligned take the scalar path."""
    lse, s = kernel_case(1030, 9)
    lse_t = torch.from_numpy(lse).cuda()[1:]
    s_t = torch.from_numpy(s).cuda()[1:]
    lns_t = torch.log(s_t)
    out = torch.empty(1030, device="cuda")[1:]
    lik = F.event_weight_lse(lse_t, s_t, lns_t, out, True)
    want = lse_t - lns_t
    want[s_t == 0] = INF
    assert torch.equal(out, want)
    lik_a = F.event_weight_lse(lse_t.clone(), s_t.clone(), lns_t.clone(),
                               torch.empty(1029, device="cuda"), True)
    live = s[1:] != 0
    terms = s[1:][live].astype(np.float64) * lse[1:][live].astype(np.float64)
    assert abs(float(lik.item()) - terms.sum()) <= lik_bound(1029, terms)
    assert abs(float(lik_a.item()) - terms.sum()) <= lik_bound(1029, terms)


# ----------------------------------------------------------------- engine

def cfg_for(k, iters, **kw):
    return GmmConfig(num_clusters=k, target_num_clusters=k,
                     min_iters=iters, max_iters=iters, **kw)


def params(eng, k):
    st = eng.state.shrink(k)
    return {q: getattr(st, q).detach().cpu().clone()
            for q in ("N", "means", "R", "pi")}


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_ones_weights_bitwise_equal_lse_path(dtype):
    data, _ = make_supported_blobs(1500, 5, 4, seed=21)
    cfg = cfg_for(4, 3, estep_dtype=dtype)
    eng_w = build_engine(data, cfg, device="cuda",
                         weights=np.ones(1500, np.float32))
    assert eng_w.use_graphs and not eng_w.use_lds_estep
    eng_u = build_engine(data, cfg, device="cuda")
    assert eng_u._lse_w is None and eng_u.s is None
    eng_u.use_lds_estep = False
    lik_w = eng_w.run_em(4)
    lik_u = eng_u.run_em(4)
    # iterations 2 and 3 ran from captured graphs (2 is a replay)
    assert eng_w._graphs and all(eng_w._graphs.values())
    a, b = params(eng_w, 4), params(eng_u, 4)
    for q in a:
        assert torch.equal(a[q], b[q]), q
    assert torch.equal(eng_w._lse, eng_u._lse)
    assert torch.equal(eng_w._lse_w, eng_w._lse)
    lse64 = eng_w._lse.double().cpu().numpy()
    bound = lik_bound(1500, lse64)
    print(f"{dtype}: lik {lik_w!r} vs {lik_u!r} vs {lse64.sum()!r}, "
          f"bound {bound:.3e}")
    assert abs(lik_w - lse64.sum()) <= bound
    assert abs(lik_w - lik_u) <= bound


def weighted_blobs(n, d, k, seed):
    """Well-separated blobs with weights in {0, 0.5, 1, 2.5}, rows arranged
    so that every blob receives one strided seed. The seeds stride over the
    events with s > 0, so make_supported_blobs' own arrangement (made for
    all rows) is redone for those: a blob without a seed is shared between
    two clusters with a soft boundary, and such a fit amplifies the bf16
    rounding of the E-step beyond what the CPU comparison allows for."""
    data, labels = make_supported_blobs(n, d, k, seed=seed)
    s = np.random.default_rng(seed).choice(
        np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=n)
    keep = np.nonzero(s > 0)[0]
    stride = (len(keep) - 1.0) / (k - 1.0)
    seeds = [int(keep[int(c * stride)]) for c in range(k)]
    for c, p in enumerate(seeds):
        if labels[p] == c:
            continue
        q = next(int(j) for j in keep
                 if labels[j] == c and int(j) not in seeds)
        data[[p, q]] = data[[q, p]]
        labels[[p, q]] = labels[[q, p]]
    return data, s


_cases = {}


def weighted_case(d, k, diag=False):
    """Data, weights and the weighted CPU fit, computed once per shape."""
    key = (d, k, diag)
    if key not in _cases:
        data, s = weighted_blobs(1500, d, k, seed=31 + d)
        eng = build_engine(data, cfg_for(k, 5, diag_only=diag), device="cpu",
                           weights=s)
        lik = eng.run_em(k)
        _cases[key] = (data, s, params(eng, k), lik)
    return _cases[key]


@pytest.mark.parametrize("path,d,k,dtype", [
    ("fused", 5, 4, "bf16"), ("fused", 5, 4, "fp32"),
    ("big", 40, 3, "bf16"), ("big", 40, 3, "fp32"),
    ("valu", 5, 4, "fp32"), ("diag", 5, 4, "fp32"),
])
def test_weighted_em_gpu_matches_cpu(path, d, k, dtype):
    diag = path == "diag"
    data, s, ref, lik_c = weighted_case(d, k, diag)
    eng = build_engine(data, cfg_for(k, 5, estep_dtype=dtype, diag_only=diag),
                       device="cuda", weights=s)
    if path == "valu":
        eng.use_fused_estep = False
        eng.mfac32 = None
    assert not eng.use_lds_estep
    assert eng.use_fused_estep == (path in ("fused", "diag"))
    assert eng.use_big_estep == (path == "big")
    assert eng.n_total == pytest.approx(float(s.astype(np.float64).sum()))
    lik_g = eng.run_em(k)
    got = params(eng, k)
    print(f"{path}/{dtype}: lik gpu {lik_g!r} cpu {lik_c!r}; max dN "
          f"{float((got['N'] - ref['N']).abs().max()):.3e}")
    # the tolerances of test_gpu_engine.py::test_em_gpu_matches_cpu
    np.testing.assert_allclose(got["N"].numpy(), ref["N"].numpy(), rtol=1e-3)
    np.testing.assert_allclose(got["means"].numpy(), ref["means"].numpy(),
                               rtol=1e-2, atol=1e-2)
    np.testing.assert_allclose(got["R"].numpy(), ref["R"].numpy(),
                               rtol=5e-2, atol=5e-2)


def test_posteriors_stay_normalised_and_zero_weight_is_exact():
    data, s, _, _ = weighted_case(5, 4)
    cfg = cfg_for(4, 3)
    eng = build_engine(data, cfg, device="cuda", weights=s)
    eng.run_em(4)
    post = eng.posteriors(4)
    assert post.shape == (4, 1500)
    assert float((post.sum(dim=0) - 1.0).abs().max()) <= 1e-5
    # the staged weight of a zero-weight event is an exact 0
    assert bool((eng._lse_w[eng.s == 0] == INF).all())
    assert bool((torch.exp(eng.w[:4] - eng._lse_w)[:, eng.s == 0] == 0).all())
    # ... so garbage in its data changes no cluster's N (nor anything else)
    garbage = data.copy()
    zero_rows = np.nonzero(s == 0)[0]
    garbage[zero_rows[3]] = 9.0e3
    garbage[zero_rows[4]] = -4.0e3
    eng_g = build_engine(garbage, cfg, device="cuda", weights=s)
    eng_g.run_em(4)
    a, b = params(eng, 4), params(eng_g, 4)
    for q in a:
        assert torch.equal(a[q], b[q]), q
    w = eng.recompute_memberships(eng.state.shrink(4))
    assert float((w.sum(dim=0) - 1.0).abs().max()) <= 1e-5


def test_weighted_sweep_k_sequence_matches_cpu():
    data, s = weighted_blobs(1500, 3, 3, seed=41)
    cfg = GmmConfig(num_clusters=5, target_num_clusters=2,
                    min_iters=5, max_iters=5)
    res_c = build_engine(data, cfg, device="cpu", weights=s).sweep()
    res_g = build_engine(data, cfg, device="cuda", weights=s).sweep()
    print("K sequence cpu", sorted(res_c.rissanen_by_k),
          "gpu", sorted(res_g.rissanen_by_k))
    assert sorted(res_g.rissanen_by_k) == sorted(res_c.rissanen_by_k)
    assert res_g.num_clusters == res_c.num_clusters
