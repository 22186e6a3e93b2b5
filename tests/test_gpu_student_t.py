"""Student-t mixture components on the GPU: student_t_lse and student_t_pi
against the float64 oracle of student_t_oracle.py, the engine on every
E-step path against the CPU engine, graph replay against eager launches,
the off switch, and predict on cuda against cpu. Every check prints its
figure next to the bound before it asserts."""
import numpy as np
import pytest
import torch

import student_t_oracle as so

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.engine import build_engine  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402
from cuda_gmm_mpi_amd.utils.config import GmmConfig  # noqa: E402

INF = float("inf")
NAN = float("nan")
U32 = 2.0 ** -24   # fp32 unit roundoff
DEV = "cuda"
D = 24             # enters the kernel only as a scalar

SIZES = [1, 63, 1024, 4097, 8195]
KS = [1, 3, 64, 105]
NUS = [1.0, 4.0, 1e4]


def kernel_case(n, k, dead=True):
    """fp32 (logw, add, s) with logw = add_c - q/2 built from chosen q:
    chi-square-like values on three scales plus 0, 1e6 and +inf; with
    `dead` one event whose q are all +inf; one event with s = 0."""
    rng = np.random.default_rng([17, n, k])
    add = rng.uniform(-30.0, -5.0, k).astype(np.float32)
    q = (rng.chisquare(D, (k, n))
         * rng.choice([0.2, 1.0, 30.0], (k, n))).astype(np.float32)
    s = rng.choice(np.array([0.5, 1.0, 2.5], np.float32), size=n)
    if n >= 8:
        q[0, 0], q[k // 2, 1], q[k - 1, 2] = 0.0, 1e6, INF
        if dead:
            q[:, n // 2] = INF
        s[n // 3] = 0.0
    logw = add[:, None] - np.float32(0.5) * q
    return logw.astype(np.float32), add, s


def run_kernel(logw, add, nu, s=None, train=True, lik=True):
    """One launch at the extension on NaN-prefilled outputs. Returns a dict
    of CPU tensors / float64 arrays."""
    ext = hip_ext()
    k, n = logw.shape
    lw = torch.from_numpy(logw).to(DEV)
    add_t = torch.from_numpy(add).to(DEV)
    empty = lw.new_empty(0)
    blocks = int(ext.student_t_lse_blocks(n))
    lse_t = torch.full((n,), NAN, device=DEV)
    if train:
        s_t = torch.from_numpy(s).to(DEV) if s is not None else empty
        lns = torch.log(s_t) if s is not None else empty
        lse_m = torch.full((n,), NAN, device=DEV)
        n_part = torch.full((blocks, k), NAN, device=DEV)
        lik_part = torch.full((blocks,), NAN, device=DEV) if lik else empty
    else:
        s_t = lns = lse_m = n_part = lik_part = empty
    ext.student_t_lse(lw, add_t, s_t, lns, lse_m, lse_t, n_part, lik_part,
                      float(nu), D, so.delta(nu, D), train)
    torch.cuda.synchronize()
    assert torch.equal(add_t.cpu(), torch.from_numpy(add))
    res = {"out": lw.cpu(), "lse_t": lse_t.cpu()}
    assert not bool(torch.isnan(res["out"]).any())
    assert not bool(torch.isnan(res["lse_t"]).any())
    if train:
        assert not bool(torch.isnan(n_part).any()), "an unwritten n_part slot"
        assert not bool(torch.isnan(lik_part).any()), "an unwritten lik slot"
        assert not bool(torch.isnan(lse_m).any())
        res.update(lse_m=lse_m.cpu(),
                   n_part=n_part.cpu().numpy().astype(np.float64),
                   lik_part=(lik_part.cpu().numpy().astype(np.float64)
                             if lik else None))
    return res


def tiles_per_block(n):
    """Tiles one block walks: 16-byte tiles of 1024 events when n % 4 == 0,
    else scalar tiles of 256; one block per 1024 events, at most 2048."""
    blocks = max(1, min((n + 1023) // 1024, 2048))
    tiles = n // 1024 + (n % 1024 > 0) if n % 4 == 0 else -(-n // 256)
    return -(-tiles // blocks)


# Error model of the kernel against the float64 contract on the SAME fp32
# inputs, in units of u = 2^-24, with a = add_c + delta, h = (nu + D)/2 and
# P = h log1p(q / nu), so that lt = a - P:
#   q: one rounded subtraction (the doubling is exact), relative u; the
#   division by nu another u. log1p turns a relative change r of q / nu into
#   at most r x/(1 + x) <= r log1p(x), and log1pf itself is good to 2 ulp =
#   4 u of its value; h is rounded (u) and so is the product (u): 8 u P.
#   a: delta rounded to fp32, u |delta|, and one addition, u |a|; the final
#   subtraction u |lt|. Both a and lt can cancel (delta is +26 at nu = 1
#   against add down to -30), so these are u of the terms, not of the value.
# So |d lt| <= 8 u max(1, |add_c| + |delta| + P): the 4 u max(1, |value|)
# rule with the value replaced by the size of the terms it is the sum of,
# and 8 for 4 because of log1pf's 2 ulp times h.
# Train mode adds ln u = logf(fl(nud / fl(nu + q))): argument good to 3 u,
# logf to 2 u of its value, one more addition: the same rule with |ln u|
# added to the scale.
# lse_t = logsumexp: d lse <= sum_c tau_c |d lt_c| + the recurrence's own
# error, at most 2 u per expf and u per addition on a sum >= 1, and logf:
# (2 K + 8) u.
def lt_scale(ref, add, nu, train):
    h = 0.5 * (nu + D)
    with np.errstate(invalid="ignore", over="ignore"):
        sc = (np.abs(add.astype(np.float64)[:, None]) + abs(so.delta(nu, D))
              + h * np.log1p(ref["q"] / nu))
        if train:
            sc = sc + np.abs(ref["lnu"])
    return sc


def check_values(label, got, want, tol):
    got = got.numpy().astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), f"{label}: infinities"
    if not fin.any():
        return
    ratio = float((np.abs(got[fin] - want.astype(np.float32)
                          .astype(np.float64)[fin])
                   / (tol[fin] + U32 * np.abs(want[fin]))).max())
    print(f"ST {label}: err/tol {ratio:.3f}")
    assert ratio <= 1.0, (label, ratio)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_student_t_lse_vs_oracle(n, k):
    logw, add, s = kernel_case(n, k)
    for nu in NUS:
        post = run_kernel(logw, add, nu, train=False)
        refp = so.student_t_lse(logw, add, nu, D, train=False)
        tol_lt = 8 * U32 * np.maximum(1.0, lt_scale(refp, add, nu, False))
        check_values(f"posterior out n={n} K={k} nu={nu:g}", post["out"],
                     refp["out"], tol_lt)
        for weighted in (False, True):
            tag = f"n={n} K={k} nu={nu:g} w={weighted}"
            sw = s if weighted else None
            ref = so.student_t_lse(logw, add, nu, D, sw)
            got = run_kernel(logw, add, nu, sw)
            tol_out = 8 * U32 * np.maximum(1.0, lt_scale(ref, add, nu, True))
            check_values(f"out {tag}", got["out"], ref["out"], tol_out)
            with np.errstate(invalid="ignore"):
                tau = np.exp(ref["lt"] - ref["lse_t"])
            tau = np.where(np.isfinite(tau), tau, 0.0)
            tol_lse = ((tau * np.where(np.isfinite(tol_lt), tol_lt, 0.0))
                       .sum(axis=0) + (2 * k + 8) * U32)
            check_values(f"lse_t {tag}", got["lse_t"], ref["lse_t"], tol_lse)
            check_values(f"lse_m {tag}", got["lse_m"], ref["lse_m"], tol_lse)
            check_values(f"posterior lse_t {tag}", post["lse_t"],
                         ref["lse_t"], tol_lse)
            if weighted:
                # bitwise event_weight_lse of the kernel's own lse_t
                s_t = torch.from_numpy(s).to(DEV)
                ew = torch.empty(n, device=DEV)
                F.event_weight_lse(got["lse_t"].to(DEV), s_t, torch.log(s_t),
                                   ew, False)
                assert torch.equal(ew.cpu(), got["lse_m"]), tag
                assert bool((got["lse_m"][torch.from_numpy(s == 0)]
                             == INF).all())
            else:
                assert torch.equal(got["lse_m"], got["lse_t"])
            if n >= 8:      # the event with every q = +inf
                assert float(got["lse_t"][n // 2]) == -INF
                assert bool((got["out"][:, n // 2] == -INF).all())
            # ---- n_part: (adds per thread + 10) u sum |terms| for the
            # summation (4 events of a tile, a 6-step wave tree, one add
            # into the table per tile, 4 waves), plus what the terms
            # s exp(lt - lse_t) inherit from lt and lse_t and expf's 2 u;
            # a term below the smallest normal fp32 may be flushed to zero
            adds = 4 + 6 + tiles_per_block(n) + 4
            terms = ref["tau_s"]
            inherit = (terms * (np.where(np.isfinite(tol_lt), tol_lt, 0.0)
                                + tol_lse[None, :] + 4 * U32)).sum(axis=1)
            bound = (U32 * (adds + 10) * terms.sum(axis=1) + inherit
                     + 2.0 ** -126 * n * 2.5)
            n_c = got["n_part"].sum(axis=0)
            ratio = float((np.abs(n_c - ref["n_c"])
                           / np.maximum(bound, 1e-300)).max())
            print(f"ST n_part {tag}: sum {n_c.sum():.6f} want "
                  f"{ref['n_c'].sum():.6f} err/tol {ratio:.3f}")
            assert ratio <= 1.0
            # a live event at -inf makes the likelihood -inf, as plain EM's
            live = (s > 0) if weighted else np.ones(n, bool)
            if n >= 8 and live[n // 2]:
                assert got["lik_part"].sum() == -INF


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_student_t_lse_likelihood_partials(n, weighted):
    """The finite case: no event at -inf. (adds per thread + 10) u
    sum |terms| on the kernel's own lse_t, as for background_lse."""
    k, nu = 3, 4.0
    logw, add, s = kernel_case(n, k, dead=False)
    got = run_kernel(logw, add, nu, s if weighted else None)
    lt64 = got["lse_t"].numpy().astype(np.float64)
    sw = s.astype(np.float64) if weighted else np.ones(n)
    live = sw > 0
    terms = sw[live] * lt64[live]
    adds = 4 * tiles_per_block(n) + 6 + 4 + (1 if weighted else 0)
    bound = U32 * (adds + 10) * np.abs(terms).sum()
    diff = abs(got["lik_part"].sum() - terms.sum())
    print(f"ST lik n={n} w={weighted}: got {got['lik_part'].sum()!r} want "
          f"{terms.sum()!r} err/tol {diff / bound if bound else 0.0:.3f}")
    assert diff <= bound
    # without the likelihood the other outputs are bitwise the same
    off = run_kernel(logw, add, nu, s if weighted else None, lik=False)
    assert off["lik_part"] is None
    assert torch.equal(off["out"], got["out"])
    assert np.array_equal(off["n_part"], got["n_part"])


def test_student_t_lse_deterministic_unaligned_and_checks():
    n, k, nu = 8195, 64, 4.0
    logw, add, s = kernel_case(n, k)
    a = run_kernel(logw, add, nu, s)
    b = run_kernel(logw, add, nu, s)
    for q in ("out", "lse_t", "lse_m"):
        assert torch.equal(a[q], b[q]), q
    assert np.array_equal(a["n_part"], b["n_part"])
    assert np.array_equal(a["lik_part"], b["lik_part"])
    # n % 4 == 0 takes the 16-byte path, a view offset by one float the
    # scalar one: elementwise outputs are bitwise equal
    n4 = 4096
    lw4, add4, _ = kernel_case(n4, 3)
    vec = run_kernel(lw4, add4, nu)
    ext = hip_ext()
    buf = torch.full((3 * n4 + 1,), NAN, device=DEV)
    view = buf[1:].view(3, n4)
    view.copy_(torch.from_numpy(lw4))
    lse_t = torch.empty(n4, device=DEV)
    lse_m = torch.empty(n4, device=DEV)
    blocks = int(ext.student_t_lse_blocks(n4))
    n_part = torch.full((blocks, 3), NAN, device=DEV)
    empty = buf.new_empty(0)
    ext.student_t_lse(view, torch.from_numpy(add4).to(DEV), empty, empty,
                      lse_m, lse_t, n_part, empty, nu, D, so.delta(nu, D),
                      True)
    assert torch.equal(view.cpu(), vec["out"])
    assert torch.equal(lse_t.cpu(), vec["lse_t"])
    assert bool(torch.isnan(buf[0]))
    np.testing.assert_allclose(n_part.cpu().numpy().sum(axis=0),
                               vec["n_part"].sum(axis=0), rtol=80 * U32)
    # argument checks happen before the launch
    lw = torch.from_numpy(logw).to(DEV)
    add_t = torch.from_numpy(add).to(DEV)
    lse = torch.empty(n, device=DEV)
    good = torch.empty(int(ext.student_t_lse_blocks(n)), k, device=DEV)
    dl = so.delta(nu, D)
    with pytest.raises(RuntimeError):   # n_part of another size
        ext.student_t_lse(lw, add_t, empty, empty, lse, lse.clone(),
                          good[:-1], empty, nu, D, dl, True)
    with pytest.raises(RuntimeError):   # short lse_t
        ext.student_t_lse(lw, add_t, empty, empty, lse, lse[:-1].clone(),
                          good, empty, nu, D, dl, True)
    with pytest.raises(RuntimeError):   # s without lns
        ext.student_t_lse(lw, add_t, lse, empty, lse, lse.clone(), good,
                          empty, nu, D, dl, True)
    with pytest.raises(RuntimeError):   # nu = 0
        ext.student_t_lse(lw, add_t, empty, empty, lse, lse.clone(), good,
                          empty, 0.0, D, dl, True)
    with pytest.raises(RuntimeError):   # posterior mode takes no partials
        ext.student_t_lse(lw, add_t, empty, empty, empty, lse, good, empty,
                          nu, D, dl, False)


def test_functional_train_and_posterior():
    n, k, nu = 4097, 3, 4.0
    logw, add, s = kernel_case(n, k, dead=False)
    ref = so.student_t_lse(logw, add, nu, D, s)
    lw = torch.from_numpy(logw).to(DEV)
    add_t = torch.from_numpy(add).to(DEV)
    s_t = torch.from_numpy(s).to(DEV)
    # buffers sized for a larger starting K, as in a sweep
    n_part, lik_part = F.student_t_partials(n, k + 2, DEV)
    lse_m, lse_t = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    n_c = torch.full((k,), NAN, device=DEV)
    sentinel = torch.full((1,), -4242.0, device=DEV)
    assert F.student_t_lse(lw.clone(), add_t, nu, D, s_t, torch.log(s_t),
                           lse_m, lse_t, n_part, lik_part, n_c,
                           need_lik=False, lik_out=sentinel) is None
    assert float(sentinel.item()) == -4242.0
    lik = F.student_t_lse(lw.clone(), add_t, nu, D, s_t, torch.log(s_t),
                          lse_m, lse_t, n_part, lik_part, n_c,
                          lik_out=sentinel)
    assert lik.data_ptr() == sentinel.data_ptr()
    assert float(lik.item()) == pytest.approx(ref["lik"], rel=1e-5)
    np.testing.assert_allclose(n_c.cpu().numpy(), ref["n_c"], rtol=1e-5)
    tau, lse_p = F.student_t_posteriors(lw.clone(), add_t, nu, D)
    assert torch.equal(lse_p, lse_t)
    assert float((tau.sum(dim=0) - 1.0).abs().max()) <= 1e-5
    with np.errstate(invalid="ignore"):
        want = np.exp(ref["lt"] - ref["lse_t"])
    np.testing.assert_allclose(tau.cpu().numpy(), want, atol=1e-5)


@pytest.mark.parametrize("k", [1, 3, 64, 257])
def test_student_t_pi_vs_oracle(k):
    rng = np.random.default_rng(k)
    n_c = rng.uniform(1.0, 500.0, k).astype(np.float32)
    if k > 1:
        n_c[k // 2] = 0.25          # an emptied cluster: the 1e-10 floor
    const = rng.uniform(-40, -10, k).astype(np.float32)
    n_t = torch.from_numpy(n_c).to(DEV)
    n_out = torch.full((k,), NAN, device=DEV)
    pi = torch.full((k,), NAN, device=DEV)
    add = torch.full((k,), NAN, device=DEV)
    F.student_t_pi(n_t, torch.from_numpy(const).to(DEV), n_out, pi, add)
    _, rpi, radd = so.student_t_pi(n_c, const)
    assert torch.equal(n_out, n_t)
    # the total is one fp32 accumulator over K terms, then one division
    rel = (k + 2) * U32
    err_pi = float(np.abs(pi.cpu().numpy() / rpi - 1.0).max())
    err_add = float(np.abs(add.cpu().numpy() - radd).max())
    tol_add = rel + 2 * U32 + 2 * U32 * float(np.abs(radd).max())
    print(f"ST pi K={k}: rel err {err_pi:.3e} (bound {rel:.3e}), add err "
          f"{err_add:.3e} (bound {tol_add:.3e})")
    assert err_pi <= rel and err_add <= tol_add
    if k > 1:
        assert float(pi[k // 2]) == np.float32(1e-10)
    # without an add buffer nothing else is touched
    pi2 = torch.full((k,), NAN, device=DEV)
    F.student_t_pi(n_t, None, n_out, pi2)
    assert torch.equal(pi2, pi)


# ----------------------------------------------------------------- engine
K4 = 4
ENGINE_ITERS = 6
# the bands of test_gpu_background.py's cuda-against-cpu comparison
BANDS = {"bf16": dict(rtol=5e-2, atol=2e-2),
         "fp32": dict(rtol=2e-3, atol=2e-4)}


def cfg_for(k, iters, **kw):
    return GmmConfig(num_clusters=k, target_num_clusters=k,
                     min_iters=iters, max_iters=iters, **kw)


def params(eng, k):
    st = eng.state.shrink(k)
    return {q: getattr(st, q).detach().cpu().clone()
            for q in ("N", "means", "R", "pi")}


_cases = {}


def engine_case(d, weighted=False):
    """Four t3 blobs (N = 3000, K = 4), weights in {0, 0.5, 1, 2.5} when
    asked, and the CPU fit at nu = 4, computed once per shape."""
    key = (d, weighted)
    if key not in _cases:
        data, _ = so.t_blobs(20 + d, d)
        s = None
        if weighted:
            s = np.random.default_rng(d).choice(
                np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=len(data))
        eng = build_engine(data, cfg_for(K4, ENGINE_ITERS, student_t_nu=4.0),
                           device="cpu", weights=s)
        lik = eng.run_em(K4)
        _cases[key] = (data, s, params(eng, K4), lik)
    return _cases[key]


def check_engine(path, d, dtype, weighted):
    data, s, ref, lik_c = engine_case(d, weighted)
    eng = build_engine(data, cfg_for(K4, ENGINE_ITERS, student_t_nu=4.0,
                                     estep_dtype=dtype),
                       device=DEV, weights=s)
    if path == "valu":
        eng.use_fused_estep = False
        eng.mfac32 = None
    assert not eng.use_lds_estep
    assert eng.use_fused_estep == (path == "fused")
    assert eng.use_big_estep == (path == "big")
    lik_g = eng.run_em(K4)
    assert eng._graphs and all(eng._graphs.values())
    got = params(eng, K4)
    print(f"ST engine {path}/{dtype} D={d} w={weighted}: lik gpu {lik_g!r} "
          f"cpu {lik_c!r}; max dN "
          f"{float((got['N'] - ref['N']).abs().max()):.3e} max dR "
          f"{float((got['R'] - ref['R']).abs().max()):.3e}")
    band = BANDS[dtype]
    np.testing.assert_allclose(lik_g, lik_c, **band)
    for q in ("N", "means", "R", "pi"):
        np.testing.assert_allclose(got[q].numpy(), ref[q].numpy(), **band,
                                   err_msg=q)
    total = float(s.sum()) if weighted else float(data.shape[0])
    assert float(got["N"].sum()) == pytest.approx(total, rel=1e-5)
    post = eng.posteriors(K4)
    assert post.shape == (K4, data.shape[0])
    dev = float((post.sum(dim=0) - 1.0).abs().max())
    print(f"   posteriors() columns sum to 1 within {dev:.2e}")
    assert dev <= 1e-4
    if weighted:
        assert bool((eng._lse_w[eng.s == 0] == INF).all())
    return eng


@pytest.mark.parametrize("path,d,dtype", [
    ("fused", 4, "bf16"), ("fused", 4, "fp32"),
    ("fused", 24, "bf16"), ("fused", 24, "fp32"),
    ("big", 40, "bf16"), ("big", 40, "fp32"),
    ("valu", 4, "fp32"),
])
def test_student_t_em_gpu_matches_cpu(path, d, dtype):
    check_engine(path, d, dtype, weighted=False)


@pytest.mark.parametrize("path,d,dtype", [
    ("fused", 4, "bf16"), ("fused", 4, "fp32"),
    ("fused", 24, "bf16"), ("fused", 24, "fp32"),
    ("big", 40, "bf16"), ("big", 40, "fp32"),
    ("valu", 4, "fp32"),
])
def test_student_t_weighted_em_gpu_matches_cpu(path, d, dtype):
    check_engine(path, d, dtype, weighted=True)


def run_fit(data, cfg):
    eng = build_engine(data, cfg, device=DEV)
    lik = eng.run_em(cfg.num_clusters)
    torch.cuda.synchronize()
    return eng, lik


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_graph_replay_bitwise_equals_eager(monkeypatch, dtype):
    data = engine_case(4)[0]
    cfg = cfg_for(K4, ENGINE_ITERS, student_t_nu=4.0, estep_dtype=dtype)
    monkeypatch.delenv("GMM_NO_GRAPHS", raising=False)
    eng_g, lik_g = run_fit(data, cfg)
    assert eng_g._graphs and all(eng_g._graphs.values())
    monkeypatch.setenv("GMM_NO_GRAPHS", "1")
    eng_e, lik_e = run_fit(data, cfg)
    assert not eng_e._graphs
    print(f"ST graphs {dtype}: lik {lik_g!r} / {lik_e!r}")
    assert lik_g == lik_e
    a, b = params(eng_g, K4), params(eng_e, K4)
    for q in a:
        assert torch.equal(a[q], b[q]), q
    assert torch.equal(eng_g._lse_w, eng_e._lse_w)
    assert torch.equal(eng_g._t_n, eng_e._t_n)
    assert torch.equal(eng_g.w, eng_e.w)


def test_nu_zero_is_the_plain_fit(monkeypatch):
    """student_t_nu = 0 allocates and dispatches nothing: bitwise the fit of
    a config that never heard of the field, on the LDS path it keeps."""
    monkeypatch.delenv("GMM_NO_GRAPHS", raising=False)
    data = engine_case(4)[0]
    eng_off, lik_off = run_fit(data, cfg_for(K4, ENGINE_ITERS,
                                             student_t_nu=0.0,
                                             estep_dtype="bf16"))
    eng_plain, lik_plain = run_fit(data, cfg_for(K4, ENGINE_ITERS,
                                                 estep_dtype="bf16"))
    for eng in (eng_off, eng_plain):
        assert not eng.student_t
        assert eng._t_n is None and eng._lse_t is None
        assert eng._t_npart is None and eng._lse_w is None
        assert eng.use_lds_estep        # the default small-K path is kept
    assert lik_off == lik_plain
    a, b = params(eng_off, K4), params(eng_plain, K4)
    for q in a:
        assert torch.equal(a[q], b[q]), q
    assert torch.equal(eng_off.w, eng_plain.w)


# ---------------------------------------------------------------- predict
@pytest.fixture(scope="module")
def trained():
    """D = 8, K = 4, N = 3000, fitted on the CPU at nu = 4."""
    from cuda_gmm_mpi_amd.models.model import GmmModel
    data, _ = so.t_blobs(3, 8)
    eng = build_engine(data, cfg_for(K4, 8, student_t_nu=4.0), device="cpu")
    eng.run_em(K4)
    model = GmmModel.from_state(
        eng.state.shrink(K4).clone(with_memberships=False), eng.center,
        student_t_nu=4.0)
    assert model.is_student_t
    return data, model


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_cuda_matches_cpu(trained, dtype):
    data, model = trained
    ref = model.predict(data, device="cpu")
    got = model.predict(data, device=DEV, estep_dtype=dtype)
    top = np.sort(model.posteriors(data, device="cpu"), axis=0)
    gap = top[-1] - top[-2]
    # labels may differ only where the top two posteriors tie within the
    # fp32 band, whatever the E-step's dtype; on the CPU alone the share of
    # such events stays under 0.1 % on this data
    clear = gap > BANDS["fp32"]["rtol"]
    share32 = 1.0 - float(clear.mean())
    print(f"ST predict {dtype}: {100 * share32:.3f} % of the events within "
          f"the fp32 band of a tie (cap 0.1 %); "
          f"{int((got.labels != ref.labels).sum())} labels differ")
    assert share32 <= 0.001
    assert np.array_equal(got.labels[clear], ref.labels[clear])
    np.testing.assert_allclose(got.log_prob, ref.log_prob, **BANDS[dtype])
    assert got.counts.sum() == 3000 and got.background_count == 0
    post = model.posteriors(data[:500], device=DEV, estep_dtype=dtype)
    assert post.shape == (K4, 500)
    assert np.abs(post.sum(axis=0) - 1.0).max() <= 1e-4
    assert model.score(data, device=DEV, estep_dtype=dtype) == pytest.approx(
        ref.log_likelihood, rel=BANDS[dtype]["rtol"])
