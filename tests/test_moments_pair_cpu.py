"""CPU emulation of the pair-column bf16x3 moments arithmetic
(C = W . P, column p = i(i+1)/2 + j of P holding z_i z_j, z = [x; 1]) with
the kernel's bf16 rounding steps, held against float64."""
import numpy as np
import torch

from cuda_gmm_mpi_amd.ops import cpu_reference as cpu
from cuda_gmm_mpi_amd.ops import functional as F


def pair_of(p: int) -> tuple[int, int]:
    """(i, j), j <= i, of packed lower-triangle column p (integer twin of
    the kernel's tri_row_col)."""
    i = (int(np.sqrt(8.0 * p + 1.0)) - 1) // 2
    while (i + 1) * (i + 2) // 2 <= p:
        i += 1
    while i * (i + 1) // 2 > p:
        i -= 1
    return i, p - i * (i + 1) // 2


def split(v: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """fp32 -> (hi, lo) bf16 parts as fp32 values, round-to-nearest-even."""
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def emulate_pair_moments(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Packed [K, PP] moments the way the kernel forms them: x pre-split into
    bf16 planes and rebuilt as fp32 hi+lo, P = fl32(z_i z_j) split hi/lo, w
    split hi/lo, products hi.hi + (hi.lo + lo.hi) with lo.lo dropped, fp32
    accumulation."""
    d, n = x.shape
    xh, xl = F.split_bf16_planes(x)
    z = torch.cat([xh.float() + xl.float(), torch.ones(1, n)], dim=0)
    pp = (d + 1) * (d + 2) // 2
    ij = [pair_of(p) for p in range(pp)]
    ii = torch.tensor([a for a, _ in ij])
    jj = torch.tensor([b for _, b in ij])
    pm = z[ii] * z[jj]                       # [PP, N] fp32 products
    p_hi, p_lo = split(pm)
    w_hi, w_lo = split(w)
    main = w_hi @ p_hi.T
    cross = w_hi @ p_lo.T + w_lo @ p_hi.T
    return main + cross


def test_pair_map_is_inverse_of_packed_index():
    for d in range(1, 32):
        dp = d + 1
        seen = set()
        for p in range(dp * (dp + 1) // 2):
            i, j = pair_of(p)
            assert 0 <= j <= i <= d
            assert i * (i + 1) // 2 + j == p
            seen.add((i, j))
        assert len(seen) == dp * (dp + 1) // 2


def test_pair_arithmetic_matches_f64():
    """Tolerances of test_mstep_moments_b16_matches_cpu at D=24."""
    d, n, k = 24, 20000, 6
    rng = np.random.default_rng(d * 31 + 5)
    x = torch.from_numpy(rng.standard_normal((d, n)).astype(np.float32) * 3)
    w = torch.from_numpy(rng.uniform(0, 1, (k, n)).astype(np.float32))
    packed = emulate_pair_moments(x, w)
    n_c, mean_num, s = F.moments_views(packed, d)
    rn, rm, rs = cpu.mstep_sufficient_stats(x.double(), w.double())
    np.testing.assert_allclose(n_c.numpy(), rn.numpy(), rtol=1e-4)
    np.testing.assert_allclose(mean_num.numpy(), rm.numpy(),
                               rtol=3e-4, atol=1e-2)
    scale = float(rs.abs().max())
    np.testing.assert_allclose(s.numpy(), rs.numpy(),
                               rtol=3e-4, atol=3e-4 * scale)
