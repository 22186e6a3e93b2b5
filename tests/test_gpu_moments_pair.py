"""Pair-column bf16x3 moments kernel (C = W . P over lower-triangle pair
columns) against float64, against the per-cluster A = w.z kernel it
replaces as the default, and its lse / determinism / dispatch contracts.
The extension entry points are called directly so both kernels run in one
process."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.ops import cpu_reference as cpu  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

DEV = "cuda:0"


@pytest.fixture
def device():
    assert torch.cuda.is_available()
    return torch.device(DEV)


@functools.lru_cache(maxsize=None)
def case(d, k, n):
    """Seeded inputs (host + device) and the float64 reference, built once
    per shape and shared read-only between tests."""
    rng = np.random.default_rng(1000 * d + 10 * k + n)
    x = torch.from_numpy(rng.standard_normal((d, n)).astype(np.float32) * 3)
    w = torch.from_numpy(rng.uniform(0, 1, (k, n)).astype(np.float32))
    ref = cpu.mstep_sufficient_stats(x.double(), w.double())
    xd = x.to(DEV)
    return {"x": xd, "w": w.to(DEV), "split": F.split_bf16_planes(xd),
            "ref": ref}


def pack_ref(ref, d):
    """float64 (N, mean_num, S) -> packed [K, PP] rows, p = i(i+1)/2 + j."""
    n_c, mean_num, s = ref
    k = n_c.shape[0]
    t = torch.zeros(k, d + 1, d + 1, dtype=torch.float64)
    t[:, :d, :d] = s
    t[:, d, :d] = mean_num
    t[:, d, d] = n_c
    ii, jj = np.tril_indices(d + 1)
    return t[:, ii, jj]


def run(entry, split, w, lse=None, nchunk=None):
    """One moments kernel + reduce_chunks -> packed [K, PP]. The partial
    buffer starts as NaN so an unwritten entry cannot go unnoticed."""
    d, n = split[0].shape
    k = w.shape[0]
    pp = (d + 1) * (d + 2) // 2
    tiles = (n + 127) // 128
    if nchunk is None:
        nchunk = min(8, tiles)
    partials = torch.full((nchunk, k, pp), float("nan"),
                          dtype=torch.float32, device=w.device)
    lse_t = (lse if lse is not None
             else torch.empty(0, dtype=torch.float32, device=w.device))
    entry(split[0], split[1], w, lse_t, partials)
    assert bool(torch.isfinite(partials).all()), "unwritten partial entries"
    out = torch.empty((k, pp), dtype=torch.float32, device=w.device)
    hip_ext().reduce_chunks(partials, out)
    return out


def check_vs_f64(packed, ref, d):
    """Tolerances of test_mstep_moments_b16_matches_cpu."""
    n_c, mean_num, s = F.moments_views(packed, d)
    rn, rm, rs = ref
    np.testing.assert_allclose(n_c.cpu().numpy(), rn.numpy(), rtol=1e-4)
    np.testing.assert_allclose(mean_num.cpu().numpy(), rm.numpy(),
                               rtol=3e-4, atol=1e-2)
    scale = float(rs.abs().max())
    np.testing.assert_allclose(s.cpu().numpy(), rs.numpy(),
                               rtol=3e-4, atol=3e-4 * scale)


@pytest.mark.parametrize("k", [1, 6, 33, 64, 65])
@pytest.mark.parametrize("d", [1, 2, 7, 24, 31])
def test_pair_matches_f64_dk(device, d, k):
    c = case(d, k, 3001)
    packed = run(hip_ext().mstep_moments_pair_b16, c["split"], c["w"])
    check_vs_f64(packed, c["ref"], d)


@pytest.mark.parametrize("n", [1, 127, 129])
@pytest.mark.parametrize("d,k", [(24, 6), (7, 33)])
def test_pair_matches_f64_n(device, d, k, n):
    c = case(d, k, n)
    packed = run(hip_ext().mstep_moments_pair_b16, c["split"], c["w"])
    check_vs_f64(packed, c["ref"], d)


def test_pair_more_chunks_than_tiles(device):
    """Chunks that own no tile must still write zeros."""
    d, k, n = 24, 6, 129  # 2 tiles
    c = case(d, k, n)
    packed = run(hip_ext().mstep_moments_pair_b16, c["split"], c["w"],
                 nchunk=5)
    check_vs_f64(packed, c["ref"], d)


@pytest.mark.parametrize("d,n,k", [(24, 20011, 6), (31, 4097, 33)])
def test_pair_error_vs_legacy_kernel(device, d, n, k):
    """Max error against float64, normalised by max|ref|, at most 2x the
    per-cluster kernel's: both are sums of equally sized rounding terms and
    the margin covers the different accumulation order, nothing more."""
    c = case(d, k, n)
    ref = pack_ref(c["ref"], d)
    scale = float(ref.abs().max())
    new = run(hip_ext().mstep_moments_pair_b16, c["split"], c["w"])
    old = run(hip_ext().mstep_moments_b16, c["split"], c["w"])
    e_new = float((new.cpu().double() - ref).abs().max()) / scale
    e_old = float((old.cpu().double() - ref).abs().max()) / scale
    print(f"D={d} N={n} K={k}: pair {e_new:.3e}  legacy {e_old:.3e}")
    assert e_new <= 2 * e_old, (
        f"pair kernel error {e_new:.3e} > 2 x legacy error {e_old:.3e}")


@pytest.mark.parametrize("d,k,n", [(24, 6, 3001), (7, 33, 129)])
def test_pair_lse_path_bit_identical(device, d, k, n):
    """w = logw with lse given is bit-identical to the same kernel fed
    exp(logw - lse), materialised by exp_sub_lse with the kernel's own
    __expf. N is no tile multiple, so pad events must contribute nothing:
    the lse result is also held against float64."""
    c = case(d, k, n)
    rng = np.random.default_rng(7 * d + n)
    logw = torch.from_numpy(
        rng.standard_normal((k, n)).astype(np.float32) * 3).to(device)
    lse = torch.logsumexp(logw, dim=0).contiguous()
    w_mat = torch.empty_like(logw)
    hip_ext().exp_sub_lse(logw, lse, w_mat)
    entry = hip_ext().mstep_moments_pair_b16
    a = run(entry, c["split"], logw, lse=lse)
    b = run(entry, c["split"], w_mat)
    assert torch.equal(a, b)
    ref = cpu.mstep_sufficient_stats(c["x"].cpu().double(),
                                     w_mat.cpu().double())
    check_vs_f64(a, ref, d)


def test_pair_deterministic(device):
    c = case(24, 6, 20011)
    entry = hip_ext().mstep_moments_pair_b16
    a = run(entry, c["split"], c["w"])
    b = run(entry, c["split"], c["w"])
    assert torch.equal(a, b)


def test_dispatch_default_and_legacy(device, monkeypatch):
    """F.mstep_moments(precision="bf16x3") runs the pair kernel; with
    GMM_MOMENTS_B16=legacy it runs the per-cluster kernel. Both bitwise."""
    d, k, n = 24, 6, 20011
    c = case(d, k, n)
    tiles = (n + 127) // 128
    monkeypatch.delenv("GMM_MOMENTS_B16", raising=False)
    got = F.mstep_moments(c["x"], c["w"], precision="bf16x3",
                          x_split=c["split"])
    want = run(hip_ext().mstep_moments_pair_b16, c["split"], c["w"],
               nchunk=min(F.PAIR_NCHUNK, tiles))
    assert torch.equal(got, want)
    monkeypatch.setenv("GMM_MOMENTS_B16", "legacy")
    got = F.mstep_moments(c["x"], c["w"], precision="bf16x3",
                          x_split=c["split"])
    want = run(hip_ext().mstep_moments_b16, c["split"], c["w"],
               nchunk=min(256, tiles))
    assert torch.equal(got, want)
