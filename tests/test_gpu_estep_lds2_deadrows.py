"""estep_fused_lds2 sums only the accumulator registers that hold factor
rows below d, NL = 4 ceil(d / 8) of 16, chosen by the launcher. The rows
left out are exact zeros, so `w` and `partial` must stay bit-identical to
fixtures dumped from the commit before (scripts/dump_mstep_tail_golden.py).

d sits on both sides of every NL boundary (8, 16, 24; d = 24, 31 and 1 are
pinned by test_gpu_estep_family_golden.py). K = 5 gives one wave a second
cluster; n = 200 is a partial tile with n % 4 == 0 (16-byte posterior
stores), n = 131 takes the scalar store path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 5
SHAPES = [(d, 200) for d in (7, 8, 9, 15, 16, 17, 23, 25)] + [(9, 131)]


def from_bits(a, device):
    return torch.from_numpy(a.view(np.int16)).to(device).view(torch.bfloat16)


@pytest.mark.parametrize("d,n", SHAPES)
def test_lds2_live_rows_bit_identical_to_parent(d, n):
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(GOLDEN,
                             f"estep_lds2_deadrows_k{K}_d{d}_n{n}.npz"))
    z, mfac = from_bits(g["z"], dev), from_bits(g["mfac"], dev)
    add = torch.from_numpy(g["add"]).to(dev)
    assert z.shape == (d, n) and add.shape == (K,)
    # what the kernel relies on: the table is zero from row d on
    assert not g["mfac"].reshape(K, 2, 32, 32)[:, :, d:, :].any()
    w = torch.full((K, n), float("nan"), dtype=torch.float32, device=dev)
    partial = torch.full(((n + 127) // 128,), float("nan"),
                         dtype=torch.float32, device=dev)
    hip_ext().estep_fused_lds2(z, mfac, add, w, partial)
    for name, t in (("w", w), ("partial", partial)):
        got = t.cpu().numpy()
        assert np.isfinite(got).all(), f"unwritten {name}"
        assert np.array_equal(got.view(np.uint32), g[name].view(np.uint32)), \
            f"{name} differs from parent"
