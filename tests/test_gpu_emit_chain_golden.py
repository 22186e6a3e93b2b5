"""Bit-identity of emit_mfac's factor chain (Cholesky of R, triangular
inverse) against fixtures dumped from the commit before the chain moved
into registers for D <= 32 (scripts/dump_emit_chain_golden.py). The register
form gives every element the same operations in the same order, fused and
unfused alike, so every output array must match bit for bit.

mstep_finalize_emit shapes (K, D, world), each with the N = 0 and N = 0.75
rows that fe_inputs puts in: D = 2 (one chain step), D = 9 (the first
unfused eight of the inverse), D = 17 (the head length (j - i) & 7 wraps
twice), D = 32 with two ranks' ridge (the last D of the register form) and
D = 33 (the first D of the general form). Each runs with and without mfac32.
The per-K paths (F.constants, emit_factors) run at D = 9 and D = 32.

The clamp cases feed emit_factors an R that is not positive definite: the
identity with R[1][0] = R[0][1] = 1.0001, so that 1 - 1.0001^2 < 0 and the
second pivot is the 1e-8 * diag0 clamp under any rounding; at D = 9 and at
D = 33, and the outputs must be finite."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FE_SHAPES = [(3, 2, 1), (3, 9, 1), (3, 17, 1), (3, 32, 2), (3, 33, 1)]
PERK = [(3, 9), (3, 32)]
CLAMP_D = [9, 33]


def bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def nans(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def nan_mfac(dev, k, d):
    _, rows, cols = F.mfac_shape(d)
    return torch.full((k, 2, rows, cols), float("nan"), dtype=torch.bfloat16,
                      device=dev)


def opt_mfac32(dev, k, d, with32):
    _, rows, cols = F.mfac_shape(d)
    return (nans(dev, k, rows, cols) if with32
            else torch.empty(0, dtype=torch.float32, device=dev))


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    if got.dtype == np.float32:
        assert np.isfinite(got).all(), f"unwritten {what}"
        got, want = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(got, want), f"{what} differs from parent"


def load(k, d, world):
    return np.load(os.path.join(GOLDEN,
                                f"emit_chain_fe_k{k}_d{d}_w{world}.npz"))


WITH32 = pytest.mark.parametrize("with32", [True, False],
                                 ids=["mfac32", "bf16only"])


@WITH32
@pytest.mark.parametrize("k,d,world", FE_SHAPES)
def test_finalize_emit_bit_identical_to_parent(k, d, world, with32):
    dev = torch.device("cuda:0")
    g = load(k, d, world)
    packed = g["packed"]
    assert packed.shape == (k, (d + 1) * (d + 2) // 2)
    assert not packed[k - 1].any()           # the N = 0 row
    assert 0.5 < packed[k - 2, -1] < 1.0     # the N = 0.75 row
    out = {"N": nans(dev, k), "means": nans(dev, k, d),
           "R": nans(dev, k, d, d), "pi": nans(dev, k),
           "constant": nans(dev, k), "add": nans(dev, k)}
    mfac, mfac32 = nan_mfac(dev, k, d), opt_mfac32(dev, k, d, with32)
    hip_ext().mstep_finalize_emit(
        torch.from_numpy(packed).to(dev), torch.from_numpy(g["avgvar"]).to(dev),
        world, out["N"], out["means"], out["R"], out["pi"], out["constant"],
        out["add"], mfac, mfac32)
    for name, t in out.items():
        same_bits(t.cpu().numpy(), g[name], name)
    same_bits(bits(mfac), g["mfac"], "mfac")
    if with32:
        same_bits(mfac32.cpu().numpy(), g["mfac32"], "mfac32")


@WITH32
@pytest.mark.parametrize("k,d", PERK)
def test_constants_path_bit_identical_to_parent(k, d, with32):
    """F.constants: LU inverse and constants, then the shared emission."""
    dev = torch.device("cuda:0")
    g = load(k, d, 2 if d == 32 else 1)
    r, means, pi = (torch.from_numpy(g[n]).to(dev)
                    for n in ("R", "means", "pi"))
    mfac, add = nan_mfac(dev, k, d), nans(dev, k)
    mfac32 = opt_mfac32(dev, k, d, with32) if with32 else None
    rinv, const = F.constants(r, means, False, mfac, mfac32, pi_add=(pi, add),
                              out=(nans(dev, k, d, d), nans(dev, k)))
    same_bits(rinv.cpu().numpy(), g["lu_rinv"], "rinv")
    same_bits(const.cpu().numpy(), g["lu_constant"], "constant")
    same_bits(add.cpu().numpy(), g["lu_add"], "add")
    same_bits(bits(mfac), g["lu_mfac"], "mfac")
    if with32:
        same_bits(mfac32.cpu().numpy(), g["lu_mfac32"], "mfac32")


@WITH32
@pytest.mark.parametrize("k,d", PERK)
def test_emit_factors_bit_identical_to_parent(k, d, with32):
    dev = torch.device("cuda:0")
    g = load(k, d, 2 if d == 32 else 1)
    r, means, pi = (torch.from_numpy(g[n]).to(dev)
                    for n in ("R", "means", "pi"))
    mfac, mfac32 = nan_mfac(dev, k, d), opt_mfac32(dev, k, d, with32)
    const, add = nans(dev, k), nans(dev, k)
    hip_ext().emit_factors(r, means, mfac, mfac32, pi, const, add)
    same_bits(const.cpu().numpy(), g["ef_constant"], "constant")
    same_bits(add.cpu().numpy(), g["ef_add"], "add")
    same_bits(bits(mfac), g["ef_mfac"], "mfac")
    if with32:
        same_bits(mfac32.cpu().numpy(), g["ef_mfac32"], "mfac32")


@WITH32
@pytest.mark.parametrize("d", CLAMP_D)
def test_clamped_pivot_bit_identical_to_parent(d, with32):
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(GOLDEN, f"emit_chain_clamp_d{d}.npz"))
    r = g["R"]
    want = np.eye(d, dtype=np.float32)
    want[1, 0] = want[0, 1] = np.float32(1.0001)
    assert np.array_equal(r[0], want)
    # lower Cholesky by hand: L[1][0] = 1.0001, pivot^2 = 1 - L[1][0]^2 < 0
    assert np.float32(1.0) - r[0, 1, 0] * r[0, 1, 0] < 0
    rt, means, pi = (torch.from_numpy(g[n]).to(dev)
                     for n in ("R", "means", "pi"))
    mfac, mfac32 = nan_mfac(dev, 1, d), opt_mfac32(dev, 1, d, with32)
    const, add = nans(dev, 1), nans(dev, 1)
    hip_ext().emit_factors(rt, means, mfac, mfac32, pi, const, add)
    same_bits(const.cpu().numpy(), g["constant"], "constant")
    same_bits(add.cpu().numpy(), g["add"], "add")
    same_bits(bits(mfac), g["mfac"], "mfac")
    assert np.isfinite(mfac.float().cpu().numpy()).all()
    if with32:
        same_bits(mfac32.cpu().numpy(), g["mfac32"], "mfac32")
