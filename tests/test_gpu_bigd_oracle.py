"""The big-D kernels against the float64 oracles of bigd_oracle.py:
estep_logw_big (bf16 hi/lo MFMA), estep_logw_big_f32, estep_lse and
mstep_moments_big. The oracles are fed the kernels' own inputs, the
tolerances come from the fp32 reference emulations and from derivations
(bigd_oracle.py, docs/NUMERICS.md), and test_bigd_oracle_cpu.py shows on
the CPU that each would catch a dropped plane, tile, column, cross product
or cluster. Every check prints its largest error / tolerance before it
asserts."""
import numpy as np
import pytest
import torch

import bigd_oracle as bo

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def default_chunking(monkeypatch):
    """The chunk counts under test are the launchers' own unless a test
    sets them."""
    monkeypatch.delenv("GMM_BIG2_NCHUNK", raising=False)
    monkeypatch.delenv("GMM_MOMENTS_NCHUNK", raising=False)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------ E-step
def run_logw(kind, table, z, add):
    """One launch on NaN-prefilled output -> device logw [K, n]. The bf16
    casts are exact: the planes and z already hold bf16 values."""
    k, n = add.shape[0], z.shape[1]
    out = torch.full((k, n), float("nan"), dtype=torch.float32, device=DEV)
    if kind == "b16":
        F.estep_logw_big(dev(z, torch.bfloat16), dev(table, torch.bfloat16),
                         dev(add), out)
    else:
        F.estep_logw_big_f32(dev(z), dev(table), dev(add), out)
    return out


def check_logw(out, logw_ref, q_ref, eps, label):
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"{label}: unwritten or non-finite logw"
    tol = bo.logw_tolerance(eps, q_ref, logw_ref)
    ratio = float((np.abs(got - logw_ref) / tol).max())
    print(f"BIGD {label} err/tol {ratio:.3f}")
    assert ratio <= 1.0, f"{label}: error is {ratio:.2f}x the tolerance"


def run_case(kind, d, k, n):
    c = bo.estep_case(kind, d, k, n)
    out = run_logw(kind, c["table"], c["z"], c["add"])
    check_logw(out, c["logw"], c["q"], bo.estep_eps(kind, d),
               f"logw_{kind} D={d} K={k} n={n}")
    return out


@pytest.mark.parametrize("d,k,n", bo.ESTEP_B16_GRID + bo.ESTEP_B16_EDGES)
def test_estep_logw_big_vs_oracle(d, k, n):
    """KCT = 2 route (D = 12), lone augmented tile (D % 16 = 0), the tier
    edges 47/48 and 79/80, D = 96, the last D on BE = 256 and the first and
    last on BE = 128; n around one tile; K = 1."""
    run_case("b16", d, k, n)


@pytest.mark.parametrize("d,k,n", bo.ESTEP_B16_MULTI)
def test_estep_logw_big_tiles_per_block(monkeypatch, d, k, n):
    """Four z tiles walked by one block (restaging zs and qpart three
    times), by two, and one block per tile: bitwise the same logw."""
    outs = []
    for nchunk in (1, 2, 1000):
        monkeypatch.setenv("GMM_BIG2_NCHUNK", str(nchunk))
        outs.append(run_case("b16", d, k, n))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])


def test_estep_logw_big_deterministic():
    c = bo.estep_case("b16", *bo.ESTEP_B16_GRID[-1])
    a = run_logw("b16", c["table"], c["z"], c["add"])
    b = run_logw("b16", c["table"], c["z"], c["add"])
    assert torch.equal(a, b)


@pytest.mark.parametrize("d,k,n", bo.ESTEP_F32_CASES)
def test_estep_logw_big_f32_vs_oracle(d, k, n):
    run_case("f32", d, k, n)


@pytest.mark.parametrize("d", [48, 142])
def test_emitted_table_structure_and_kernels(d):
    """Coupling to emission. (a) F.constants overwrites every cell of
    NaN-prefilled tables and leaves exact zeros outside {row < d,
    col <= row} and {row < d, col = d}: the precondition that makes the
    kernels' tile skip exact. (b) Both kernels, fed that table, meet the
    oracle of that table. Nothing is claimed about the Cholesky."""
    k, n = 5, 300
    rng = np.random.default_rng([4, d])
    means, r, pi = bo.random_covariance_model(rng, k, d)
    shape = F.mfac_shape(d)
    mfac = torch.full((k, *shape), float("nan"), dtype=torch.bfloat16,
                      device=DEV)
    mfac32 = torch.full((k, *shape[1:]), float("nan"), dtype=torch.float32,
                        device=DEV)
    _, const = F.constants(dev(r), dev(means), False, mfac, mfac32)
    add = (const + torch.log(dev(pi))).cpu().numpy()
    planes = mfac.float().cpu().numpy()
    table = mfac32.cpu().numpy()
    assert np.isfinite(planes).all() and np.isfinite(table).all()
    dead = ~bo.structure_mask(d)
    assert not planes[:, :, dead].any(), "non-zero outside the structure"
    assert not table[:, dead].any(), "non-zero outside the structure"
    idx = np.arange(d)
    assert (table[:, idx, idx] > 0).all()

    z = rng.standard_normal((d, n)).astype(np.float32)
    for kind, tab, zz in (("b16", planes, bo.bf16_round(z)),
                          ("f32", table, z)):
        logw_ref, q_ref = bo.logw_oracle(tab, zz, add)
        eps = bo.eps_ref(tab, zz, add)
        out = run_logw(kind, tab, zz, add)
        check_logw(out, logw_ref, q_ref, eps, f"emitted_{kind} D={d}")


# --------------------------------------------------------------------- lse
def run_lse(logw, slots):
    n = logw.shape[1]
    lse = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    partial = torch.full((slots,), float("nan"), dtype=torch.float32,
                         device=DEV)
    hip_ext().estep_lse(dev(logw), lse, partial)
    return lse.cpu().numpy(), partial.cpu().numpy()


def check_lse(k, n, slots):
    c = bo.lse_case(k, n)
    lse, partial = run_lse(c["logw"], slots)
    assert np.isfinite(lse).all() and np.isfinite(partial).all()
    tol = bo.lse_tolerance(c["logw"], c["ref"])
    ratio = float((np.abs(lse.astype(np.float64) - c["ref"]) / tol).max())
    print(f"BIGD lse K={k} n={n} slots={slots} err/tol {ratio:.3f}")
    assert ratio <= 1.0
    # likelihood partials: each thread adds its events, then a 6-step
    # shuffle tree and 4 wave sums -> at most iters + 10 fp32 additions
    grid = min((n + 255) // 256, slots)
    iters = -(-n // (256 * grid))
    lse64 = lse.astype(np.float64)
    bound = 2.0 ** -24 * (iters + 10) * np.abs(lse64).sum()
    diff = abs(partial.astype(np.float64).sum() - lse64.sum())
    print(f"BIGD lse_partial K={k} n={n} slots={slots} "
          f"err/tol {diff / bound:.3f}")
    assert diff <= bound


@pytest.mark.parametrize("k,n", bo.LSE_CASES)
def test_estep_lse_vs_oracle(k, n):
    check_lse(k, n, (n + 255) // 256)


def test_estep_lse_grid_stride():
    """Three partial slots for five blocks' worth of events: every block
    walks a second set of events."""
    check_lse(5, 1100, 3)


# ----------------------------------------------------------------- moments
def run_moments(c, nchunk=None, w=None, lse=None):
    return F.mstep_moments(dev(c["x"]), dev(c["w"]) if w is None else w,
                           nchunk=nchunk, precision="bf16x3", lse=lse)


def check_moments(packed, ref, eps, label):
    got = packed.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    assert np.isfinite(got).all(), f"{label}: non-finite moments"
    tol = bo.moments_tolerance(eps, ref)
    ratio = float((np.abs(got - ref) / tol).max())
    print(f"BIGD {label} err/tol {ratio:.3f}")
    assert ratio <= 1.0, f"{label}: error is {ratio:.2f}x the tolerance"


@pytest.mark.parametrize("d,k,n", bo.MOMENTS_CASES)
def test_moments_big_vs_oracle(d, k, n):
    c = bo.moments_case(d, k, n)
    check_moments(run_moments(c), c["ref"], c["eps"],
                  f"moments D={d} K={k} n={n}")


@pytest.mark.parametrize("d,k,n", bo.MOMENTS_PIPE)
def test_moments_big_pipeline(d, k, n):
    """Six tiles over 1, 2, 3 and 6 chunks: the double-buffered loop runs
    6, 3, 2 and 1 tiles per block. A chunk count past the tiles is cut to
    them."""
    c = bo.moments_case(d, k, n)
    for nchunk in (1, 2, 3, 50):
        packed = run_moments(c, nchunk=nchunk)
        check_moments(packed, c["ref"], c["eps"],
                      f"moments_pipe D={d} nchunk={nchunk}")
    assert torch.equal(packed, run_moments(c, nchunk=6))


@pytest.mark.parametrize("d,k,n", [(33, 5, 329), (96, 2, 129)])
def test_moments_big_lse_staging(d, k, n):
    """w = logw with lse given is bitwise the run on exp_sub_lse's
    materialised weights (the kernel's own __expf), and meets the oracle
    of those weights; lse = +inf on every third event is bitwise the run
    with those events' weights set to 0."""
    c = bo.moments_case(d, k, n)
    rng = np.random.default_rng([5, d, n])
    logw = dev((3 * rng.standard_normal((k, n))).astype(np.float32))
    lse = torch.logsumexp(logw, dim=0).contiguous()
    w_mat = torch.empty_like(logw)
    hip_ext().exp_sub_lse(logw, lse, w_mat)
    a = run_moments(c, w=logw, lse=lse)
    assert torch.equal(a, run_moments(c, w=w_mat))
    w_np = w_mat.cpu().numpy()
    check_moments(a, bo.moments_oracle(c["x"], w_np),
                  bo.eps_mom(c["x"], w_np), f"moments_lse D={d}")

    lse_inf = lse.clone()
    lse_inf[::3] = float("inf")
    w_zero = w_mat.clone()
    w_zero[:, ::3] = 0.0
    assert torch.equal(run_moments(c, w=logw, lse=lse_inf),
                       run_moments(c, w=w_zero))


def test_moments_big_deterministic():
    c = bo.moments_case(*bo.MOMENTS_PIPE[-1])
    assert torch.equal(run_moments(c), run_moments(c))
