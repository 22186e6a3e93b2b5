"""Small-K fused E-step, second version (estep_fused_lds2) against the
kernel it replaces as the default (estep_fused_lds), against the CPU
reference, and its determinism / dispatch contracts; plus the bit-neutral
staging change of the exact-f32 sibling. The extension entry points are
called directly so both kernels run in one process."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.ops import cpu_reference as cpu  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -24

# every K and every n at D = 24; D in {1, 31} at K in {1, 9, 64} with the
# two n that have a partial tail (float4 and scalar store path)
GRID = ([(k, 24, n) for k in (1, 7, 8, 9, 64, 104)
         for n in (100, 384, 404, 313)]
        + [(k, d, n) for d in (1, 31) for k in (1, 9, 64)
           for n in (404, 313)])


@pytest.fixture
def device():
    assert torch.cuda.is_available()
    return torch.device(DEV)


def random_model(rng, k, d):
    """As in test_gpu_kernels.py."""
    means = torch.from_numpy(
        rng.standard_normal((k, d)).astype(np.float32) * 2).to(DEV)
    rs = []
    for _ in range(k):
        a = rng.standard_normal((d, d))
        rs.append((a @ a.T + d * np.eye(d)).astype(np.float32))
    r = torch.from_numpy(np.stack(rs)).to(DEV)
    pi = torch.from_numpy(
        rng.dirichlet(np.ones(k)).astype(np.float32)).to(DEV)
    return means, r, pi


def run(entry, z, mfac, add):
    """One E-step kernel into NaN-filled outputs: everything it owns must
    come back finite, so an unwritten entry cannot go unnoticed."""
    k, n = add.shape[0], z.shape[1]
    nblk = (n + 127) // 128
    w = torch.full((k, n), float("nan"), dtype=torch.float32, device=z.device)
    partial = torch.full((nblk,), float("nan"), dtype=torch.float32,
                         device=z.device)
    entry(z, mfac, add, w, partial)
    assert bool(torch.isfinite(w).all()), "unwritten posteriors"
    assert bool(torch.isfinite(partial).all()), "unwritten partials"
    return w, partial


@functools.lru_cache(maxsize=None)
def case(k, d, n):
    """Seeded inputs, the legacy kernel's output and the float64 CPU
    reference, built once per shape and shared read-only between tests."""
    rng = np.random.default_rng(100000 * d + 1000 * k + n)
    means, r, pi = random_model(rng, k, d)
    mfac = torch.empty(k, 2, 32, 32, dtype=torch.bfloat16, device=DEV)
    mfac32 = torch.empty(k, 32, 32, dtype=torch.float32, device=DEV)
    _, const_g = F.constants(r, means, False, mfac, mfac32)
    add = (const_g + torch.log(pi)).contiguous()
    x = torch.from_numpy(rng.standard_normal((d, n)).astype(np.float32) * 2)
    z = x.to(DEV).to(torch.bfloat16).contiguous()
    old_w, old_p = run(hip_ext().estep_fused_lds, z, mfac, add)
    # CPU reference on the bf16-rounded data the kernels read; it only
    # scales the likelihood bound, so its own fp32 rounding does not matter
    rinv, const = cpu.compute_constants(r.cpu())
    ref_logw = cpu.estep_logw(z.cpu().float(), means.cpu(), rinv, const,
                              pi.cpu())
    ref_lse = torch.logsumexp(ref_logw.double(), dim=0)
    return {"z": z, "mfac": mfac, "mfac32": mfac32, "add": add, "x": x,
            "means": means, "r": r, "pi": pi,
            "old_w": old_w, "old_p": old_p, "ref_lse": ref_lse}


@pytest.mark.parametrize("k,d,n", GRID)
def test_lds2_matches_legacy_kernel(device, k, d, n):
    """Both kernels on identical inputs. The per-(cluster, event)
    log-weights are bitwise equal by construction (same MFMA chain order,
    same fmaf order, commutative cross-half add), so are the per-event max
    and each exp(lw - max). What differs is the order of two sums:

    - the K-term sum of non-negative exponentials: each order is within
      (K-1) * 2^-24 relative of the exact sum, the reciprocal and the
      final multiply add one rounding each on either side, so posteriors
      agree within rtol = 2 * (K+1) * 2^-24; atol = 1e-37 covers results
      in the denormal range, whose quantum is an absolute 2^-149;
    - the 128-term sum of per-event terms max + log(total) of a block:
      the terms inherit the relative error of total as an absolute one
      (well below that relative to the term, |term| >> 1 here), and each
      summation order is within 127 * 2^-24 of the exact sum relative to
      sum |term|. Bound: (2 * (K+1) + 128) * 2^-24 * sum |term|, the sum
      of |term| taken in float64 from the CPU reference's log-weights of
      the same inputs."""
    c = case(k, d, n)
    new_w, new_p = run(hip_ext().estep_fused_lds2, c["z"], c["mfac"],
                       c["add"])
    colsum = new_w.double().sum(dim=0)
    assert float((colsum - 1.0).abs().max()) < 1e-5
    a, b = new_w.cpu().numpy(), c["old_w"].cpu().numpy()
    rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-30)
    print(f"K={k} D={d} n={n}: posterior max rel diff {rel.max():.3e} "
          f"(bound {2 * (k + 1) * EPS:.3e})")
    np.testing.assert_allclose(a, b, rtol=2 * (k + 1) * EPS, atol=1e-37)
    nblk = (n + 127) // 128
    pad = torch.zeros(nblk * 128, dtype=torch.float64)
    pad[:n] = c["ref_lse"].abs()
    scale = pad.view(nblk, 128).sum(dim=1).numpy()
    diff = np.abs(new_p.cpu().double().numpy()
                  - c["old_p"].cpu().double().numpy())
    bound = (2 * (k + 1) + 128) * EPS * scale
    print(f"  partial max diff/bound {float((diff / bound).max()):.3e}")
    assert (diff <= bound).all(), (diff, bound)


def test_lds2_matches_cpu(device):
    """Tolerances of test_estep_fused_lds_matches_cpu, same shape."""
    k, d, n = 8, 24, 20057
    c = case(k, d, n)
    rinv, const = cpu.compute_constants(c["r"].cpu())
    ref_logw = cpu.estep_logw(c["x"], c["means"].cpu(), rinv, const,
                              c["pi"].cpu())
    ref_w, ref_lik = cpu.estep_posteriors(ref_logw)
    w, partial = run(hip_ext().estep_fused_lds2, c["z"], c["mfac"], c["add"])
    np.testing.assert_allclose(w.cpu().numpy(), ref_w.numpy(),
                               rtol=5e-2, atol=2e-2)
    lik = float(partial.double().sum())
    assert lik == pytest.approx(float(ref_lik), rel=2e-3)


@pytest.mark.parametrize("k,d,n", [(64, 24, 404), (9, 31, 313)])
def test_lds2_deterministic(device, k, d, n):
    c = case(k, d, n)
    entry = hip_ext().estep_fused_lds2
    w1, p1 = run(entry, c["z"], c["mfac"], c["add"])
    w2, p2 = run(entry, c["z"], c["mfac"], c["add"])
    assert torch.equal(w1, w2)
    assert torch.equal(p1, p2)


class _Spy:
    """Forwards to the extension and records which entry points ran."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def wrapped(*args, **kwargs):
            self.calls.append(name)
            return fn(*args, **kwargs)
        return wrapped


def test_dispatch_default_and_legacy(device, monkeypatch):
    """F.estep_fused_lds runs the new kernel; with GMM_ESTEP_LDS=legacy
    the old one."""
    c = case(9, 24, 313)
    spy = _Spy(hip_ext())
    monkeypatch.setattr(F, "hip_ext", lambda: spy)
    w_out = torch.empty(9, 313, dtype=torch.float32, device=device)
    monkeypatch.delenv("GMM_ESTEP_LDS", raising=False)
    F.estep_fused_lds(c["z"], c["mfac"], c["add"], w_out, need_lik=False)
    assert spy.calls == ["estep_fused_lds2"]
    spy.calls.clear()
    monkeypatch.setenv("GMM_ESTEP_LDS", "legacy")
    w, lik = F.estep_fused_lds(c["z"], c["mfac"], c["add"], w_out)
    assert spy.calls == ["estep_fused_lds", "reduce_scalar"]
    assert torch.equal(w, c["old_w"])
    assert np.isfinite(float(lik))


def test_f32_lds_staging_bit_identical_to_parent(device):
    """estep_fused_f32_lds only had its full-tile loads hoisted ahead of
    the first wait: its output must not move by a bit. The fixture holds
    the inputs (x, mfac32, add) and the output (w, partial) of the kernel
    as it was before that change, K=9 D=24 n=313 (two full blocks and a
    tail)."""
    g = np.load(os.path.join(GOLDEN, "estep_f32_lds_k9_d24_n313.npz"))
    x = torch.from_numpy(g["x"]).to(device)
    mfac32 = torch.from_numpy(g["mfac32"]).to(device)
    add = torch.from_numpy(g["add"]).to(device)
    w, partial = run(hip_ext().estep_fused_f32_lds, x, mfac32, add)
    assert np.array_equal(w.cpu().numpy(), g["w"])
    assert np.array_equal(partial.cpu().numpy(), g["partial"])
