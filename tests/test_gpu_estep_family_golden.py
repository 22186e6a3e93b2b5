"""Bit-identity of the five small-D fused E-step kernels against fixtures
dumped from the commit before they were rebuilt from shared device pieces
(scripts/dump_estep_family_golden.py). Every kernel keeps its arithmetic
order, so every output array must match bit for bit.

Shapes (K, D, n): full tiles and a partial tail for the 128- and 256-event
kernels (at n = 257 the 256-event kernels get a tail of one event),
n % 4 != 0 and == 0, the smallest and largest D, cluster counts below,
above and not a multiple of the four waves."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# entry point -> (fixture stem, events per block)
KERNELS = {
    "estep_fused": ("estep_fused", 256),
    "estep_fused_f32": ("estep_fused_f32", 256),
    "estep_fused_lds": ("estep_fused_lds", 128),
    "estep_fused_lds2": ("estep_fused_lds2", 128),
    "estep_fused_f32_lds": ("estep_f32_lds", 128),
}
SHAPES = [(9, 24, 313), (5, 31, 257), (3, 1, 300)]


def from_bits(a, device):
    """uint16 bit patterns -> bf16 tensor."""
    return torch.from_numpy(a.view(np.int16)).to(device).view(torch.bfloat16)


@pytest.mark.parametrize("k,d,n", SHAPES)
@pytest.mark.parametrize("entry", list(KERNELS))
def test_family_bit_identical_to_parent(entry, k, d, n):
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    stem, tile = KERNELS[entry]
    g = np.load(os.path.join(GOLDEN, f"{stem}_k{k}_d{d}_n{n}.npz"))
    if "z" in g.files:
        z, fac = from_bits(g["z"], dev), from_bits(g["mfac"], dev)
    else:
        z = torch.from_numpy(g["x"]).to(dev)
        fac = torch.from_numpy(g["mfac32"]).to(dev)
    add = torch.from_numpy(g["add"]).to(dev)
    assert z.shape == (d, n) and add.shape == (k,)

    def nans(*shape):
        return torch.full(shape, float("nan"), dtype=torch.float32,
                          device=dev)
    out = {"w": nans(k, n), "partial": nans((n + tile - 1) // tile)}
    if "lse" in g.files:
        out["lse"] = nans(n)
        getattr(hip_ext(), entry)(z, fac, add, out["w"], out["lse"],
                                  out["partial"])
    else:
        getattr(hip_ext(), entry)(z, fac, add, out["w"], out["partial"])
    assert ("lse" in g.files) == (tile == 256)
    for name, t in out.items():
        got = t.cpu().numpy()
        assert np.isfinite(got).all(), f"unwritten {name}"
        assert np.array_equal(got, g[name]), f"{name} differs from parent"
