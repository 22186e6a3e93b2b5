"""Bit-identity of the M-step tail (mstep_finalize_emit, the per-K factor
and constants paths, reduce_chunks, reduce_scalar) against fixtures dumped
from the commit before its serial chains were cut
(scripts/dump_mstep_tail_golden.py). The rewrite keeps every element's
operations, their order and their fused / unfused rounding, so every output
array must match bit for bit.

mstep_finalize_emit shapes (K, D, world): the flagship D, D = 1, the
largest fused-path D with two ranks' ridge, a D below one emission item,
D past 32 (wider factor table), D = 96 (rows in two waves, the widest
table tier) and a full-covariance row at D = 70 (rows of L owned by two
waves). `packed` holds real moments; the last cluster row is all zero
(N = 0: identity reset, pi floor) and the one before it has N = 0.75
(covariance zero-gate). Each shape runs with and without mfac32."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FE_SHAPES = [(5, 24, 1), (3, 1, 1), (4, 31, 2), (2, 8, 1), (3, 40, 1),
             (2, 96, 1), (1, 70, 1)]
PERK = [(5, 24), (3, 40)]
CHUNKS_C = [1, 7, 8, 19, 256]
CHUNKS_M = 1625
SCALAR_N = [1, 255, 256, 257, 7813]


def tail_values(count, salt):
    """The dump script's input generator: float32 values of mixed sign and
    8 binades from integer arithmetic only."""
    i = np.arange(count, dtype=np.uint64) + np.uint64(salt) * np.uint64(1000003)
    h = (i * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    h = h ^ (h >> np.uint64(13))
    mant = h & np.uint64(0x007FFFFF)
    expo = np.uint64(120) + ((h >> np.uint64(23)) & np.uint64(7))
    sign = (h >> np.uint64(31)) & np.uint64(1)
    bits = (sign << np.uint64(31)) | (expo << np.uint64(23)) | mant
    return bits.astype(np.uint32).view(np.float32)


def bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def nans(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def nan_mfac(dev, k, d):
    _, rows, cols = F.mfac_shape(d)
    return torch.full((k, 2, rows, cols), float("nan"), dtype=torch.bfloat16,
                      device=dev)


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    if got.dtype == np.float32:
        assert np.isfinite(got).all(), f"unwritten {what}"
        got, want = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(got, want), f"{what} differs from parent"


def load(k, d, world):
    return np.load(os.path.join(GOLDEN,
                                f"mstep_tail_fe_k{k}_d{d}_w{world}.npz"))


@pytest.mark.parametrize("with32", [True, False], ids=["mfac32", "bf16only"])
@pytest.mark.parametrize("k,d,world", FE_SHAPES)
def test_finalize_emit_bit_identical_to_parent(k, d, world, with32):
    dev = torch.device("cuda:0")
    g = load(k, d, world)
    packed = g["packed"]
    assert packed.shape == (k, (d + 1) * (d + 2) // 2)
    if k >= 2:  # the rows the finalize rules branch on
        assert not packed[k - 1].any()
        assert 0.5 < packed[k - 2, -1] < 1.0
    _, rows, cols = F.mfac_shape(d)
    out = {"N": nans(dev, k), "means": nans(dev, k, d),
           "R": nans(dev, k, d, d), "pi": nans(dev, k),
           "constant": nans(dev, k), "add": nans(dev, k)}
    mfac = nan_mfac(dev, k, d)
    mfac32 = (nans(dev, k, rows, cols) if with32
              else torch.empty(0, dtype=torch.float32, device=dev))
    hip_ext().mstep_finalize_emit(
        torch.from_numpy(packed).to(dev), torch.from_numpy(g["avgvar"]).to(dev),
        world, out["N"], out["means"], out["R"], out["pi"], out["constant"],
        out["add"], mfac, mfac32)
    for name, t in out.items():
        same_bits(t.cpu().numpy(), g[name], name)
    same_bits(bits(mfac), g["mfac"], "mfac")
    if with32:
        same_bits(mfac32.cpu().numpy(), g["mfac32"], "mfac32")


@pytest.mark.parametrize("k,d", PERK)
def test_constants_path_bit_identical_to_parent(k, d):
    """F.constants: LU inverse and constants, then the shared emission."""
    dev = torch.device("cuda:0")
    g = load(k, d, 1)
    r, means, pi = (torch.from_numpy(g[n]).to(dev)
                    for n in ("R", "means", "pi"))
    _, rows, cols = F.mfac_shape(d)
    mfac, mfac32, add = nan_mfac(dev, k, d), nans(dev, k, rows, cols), nans(dev, k)
    rinv, const = F.constants(r, means, False, mfac, mfac32, pi_add=(pi, add),
                              out=(nans(dev, k, d, d), nans(dev, k)))
    same_bits(rinv.cpu().numpy(), g["lu_rinv"], "rinv")
    same_bits(const.cpu().numpy(), g["lu_constant"], "constant")
    same_bits(add.cpu().numpy(), g["lu_add"], "add")
    same_bits(bits(mfac), g["lu_mfac"], "mfac")
    same_bits(mfac32.cpu().numpy(), g["lu_mfac32"], "mfac32")


@pytest.mark.parametrize("k,d", PERK)
def test_emit_factors_bit_identical_to_parent(k, d):
    dev = torch.device("cuda:0")
    g = load(k, d, 1)
    r, means, pi = (torch.from_numpy(g[n]).to(dev)
                    for n in ("R", "means", "pi"))
    _, rows, cols = F.mfac_shape(d)
    mfac, mfac32 = nan_mfac(dev, k, d), nans(dev, k, rows, cols)
    const, add = nans(dev, k), nans(dev, k)
    hip_ext().emit_factors(r, means, mfac, mfac32, pi, const, add)
    same_bits(const.cpu().numpy(), g["ef_constant"], "constant")
    same_bits(add.cpu().numpy(), g["ef_add"], "add")
    same_bits(bits(mfac), g["ef_mfac"], "mfac")
    same_bits(mfac32.cpu().numpy(), g["ef_mfac32"], "mfac32")


@pytest.fixture(scope="module")
def reduce_golden():
    return np.load(os.path.join(GOLDEN, "mstep_tail_reduce.npz"))


@pytest.mark.parametrize("c", CHUNKS_C)
def test_reduce_chunks_bit_identical_to_parent(reduce_golden, c):
    """Below, at and between the 8- and 32-chunk batches, and the flagship's
    256 chunks; m = 1625 is no multiple of a block."""
    dev = torch.device("cuda:0")
    src = torch.from_numpy(
        tail_values(c * CHUNKS_M, c).reshape(c, CHUNKS_M)).to(dev)
    out = nans(dev, CHUNKS_M)
    hip_ext().reduce_chunks(src, out)
    same_bits(out.cpu().numpy(), reduce_golden[f"chunks_c{c}"], "sum")


@pytest.mark.parametrize("n", SCALAR_N)
def test_reduce_scalar_bit_identical_to_parent(reduce_golden, n):
    """One term, either side of one term per thread, and the flagship's
    7813 block partials (two batches of 16 loads, the second partial)."""
    dev = torch.device("cuda:0")
    src = torch.from_numpy(tail_values(n, 900 + n)).to(dev)
    out = nans(dev, 1)
    hip_ext().reduce_scalar(src, out)
    same_bits(out.cpu().numpy(), reduce_golden[f"scalar_n{n}"], "sum")
