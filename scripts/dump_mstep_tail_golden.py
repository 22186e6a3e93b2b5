#!/usr/bin/env python3
"""Pin the raw outputs of the M-step tail and of the lds2 E-step at the
live-row boundaries as fixtures under tests/golden/.

  mstep_tail_fe_k{K}_d{D}_w{W}.npz   mstep_finalize_emit: inputs (packed,
      avgvar) and every output (N, means, R, pi, constant, add, mfac as
      uint16 bits, mfac32). The run without mfac32 must agree with the run
      with it, so one set of arrays serves both. For the shapes in PERK the
      file also holds what the per-K paths make of that R / means / pi:
      lu_* from F.constants (LU kernel + factor emission) and ef_* from
      emit_factors.
  mstep_tail_reduce.npz              reduce_chunks / reduce_scalar outputs
      for inputs that tail_values() rebuilds from integers alone.
  estep_lds2_deadrows_k{K}_d{D}_n{N}.npz   as dump_estep_family_golden.py.

tests/test_gpu_mstep_tail_golden.py and tests/test_gpu_estep_lds2_deadrows.py
assert np.array_equal against them, so run this on the build whose behaviour
is to be pinned (the parent of a change), never on the code under test.
Existing files are not rewritten unless --force is given.

usage: python scripts/dump_mstep_tail_golden.py [--out DIR] [--force]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dump_estep_family_golden as fam  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

# (K, D, world); the last one adds a full-covariance row past one wave of
# rows (D > 64), which the two-cluster D = 96 case has no room for
FE_SHAPES = [(5, 24, 1), (3, 1, 1), (4, 31, 2), (2, 8, 1), (3, 40, 1),
             (2, 96, 1), (1, 70, 1)]
PERK = [(5, 24), (3, 40)]
CHUNKS_C = [1, 7, 8, 19, 256]
CHUNKS_M = 1625
SCALAR_N = [1, 255, 256, 257, 7813]
DEAD_K = 5
DEAD_SHAPES = [(d, 200) for d in (7, 8, 9, 15, 16, 17, 23, 25)] + [(9, 131)]


def tail_values(count, salt):
    """`count` float32 values of mixed sign and 8 binades, from integer
    arithmetic only (the same bits under every numpy)."""
    i = np.arange(count, dtype=np.uint64) + np.uint64(salt) * np.uint64(1000003)
    h = (i * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    h = h ^ (h >> np.uint64(13))
    mant = h & np.uint64(0x007FFFFF)
    expo = np.uint64(120) + ((h >> np.uint64(23)) & np.uint64(7))
    sign = (h >> np.uint64(31)) & np.uint64(1)
    bits = (sign << np.uint64(31)) | (expo << np.uint64(23)) | mant
    return bits.astype(np.uint32).view(np.float32)


def fe_inputs(k, d, world):
    """packed [K, (D+1)(D+2)/2] moments of random data under random soft
    weights (so R is positive definite), the last row all zero (N = 0) and
    the one before it scaled to N = 0.75; avgvar [K]."""
    rng = np.random.default_rng(7000 * d + 10 * k + world)
    n_ev = 40 * d + 200
    x = rng.standard_normal((n_ev, d)) * 1.5 + rng.standard_normal(d)
    xa = np.concatenate([x, np.ones((n_ev, 1))], axis=1)
    w = rng.dirichlet(np.ones(k), size=n_ev)            # [n_ev, K]
    t = np.einsum("ec,ei,ej->cij", w, xa, xa)           # [K, D+1, D+1]
    il = np.tril_indices(d)
    packed = np.concatenate(
        [t[:, il[0], il[1]], t[:, d, :d], t[:, d, d:]], axis=1)
    if k >= 2:
        packed[k - 1] = 0.0
        packed[k - 2] *= 0.75 / packed[k - 2, -1]
    avgvar = rng.uniform(0.01, 0.05, size=k)
    return packed.astype(np.float32), avgvar.astype(np.float32)


def nans(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def run_fe(packed, avgvar, world, d, with32, dev):
    """One mstep_finalize_emit call into NaN-filled outputs."""
    k = packed.shape[0]
    _, rows, cols = F.mfac_shape(d)
    out = {"N": nans(dev, k), "means": nans(dev, k, d), "R": nans(dev, k, d, d),
           "pi": nans(dev, k), "constant": nans(dev, k), "add": nans(dev, k)}
    mfac = torch.full((k, 2, rows, cols), float("nan"), dtype=torch.bfloat16,
                      device=dev)
    mfac32 = (nans(dev, k, rows, cols) if with32
              else torch.empty(0, dtype=torch.float32, device=dev))
    hip_ext().mstep_finalize_emit(
        torch.from_numpy(packed).to(dev), torch.from_numpy(avgvar).to(dev),
        world, out["N"], out["means"], out["R"], out["pi"], out["constant"],
        out["add"], mfac, mfac32)
    torch.cuda.synchronize()
    res = {name: t.cpu().numpy() for name, t in out.items()}
    res["mfac"] = fam.bits(mfac)
    if with32:
        res["mfac32"] = mfac32.cpu().numpy()
    return res


def run_perk(r, means, pi, dev):
    """The per-K paths on one (R, means, pi): F.constants and emit_factors."""
    k, d, _ = r.shape
    _, rows, cols = F.mfac_shape(d)
    rt, mt, pt = (torch.from_numpy(a).to(dev) for a in (r, means, pi))
    res = {}
    mfac = torch.full((k, 2, rows, cols), float("nan"), dtype=torch.bfloat16,
                      device=dev)
    mfac32 = nans(dev, k, rows, cols)
    add = nans(dev, k)
    rinv, const = F.constants(rt, mt, False, mfac, mfac32, pi_add=(pt, add),
                              out=(nans(dev, k, d, d), nans(dev, k)))
    torch.cuda.synchronize()
    res.update(lu_rinv=rinv.cpu().numpy(), lu_constant=const.cpu().numpy(),
               lu_add=add.cpu().numpy(), lu_mfac=fam.bits(mfac),
               lu_mfac32=mfac32.cpu().numpy())
    mfac = torch.full((k, 2, rows, cols), float("nan"), dtype=torch.bfloat16,
                      device=dev)
    mfac32, const, add = nans(dev, k, rows, cols), nans(dev, k), nans(dev, k)
    hip_ext().emit_factors(rt, mt, mfac, mfac32, pt, const, add)
    torch.cuda.synchronize()
    res.update(ef_constant=const.cpu().numpy(), ef_add=add.cpu().numpy(),
               ef_mfac=fam.bits(mfac), ef_mfac32=mfac32.cpu().numpy())
    return res


def run_reduce(dev):
    res = {}
    for c in CHUNKS_C:
        src = torch.from_numpy(
            tail_values(c * CHUNKS_M, c).reshape(c, CHUNKS_M)).to(dev)
        out = nans(dev, CHUNKS_M)
        hip_ext().reduce_chunks(src, out)
        res[f"chunks_c{c}"] = out.cpu().numpy()
    for n in SCALAR_N:
        src = torch.from_numpy(tail_values(n, 900 + n)).to(dev)
        out = nans(dev, 1)
        hip_ext().reduce_scalar(src, out)
        res[f"scalar_n{n}"] = out.cpu().numpy()
    return res


def all_finite(res, what):
    for name, a in res.items():
        if a.dtype == np.float32:
            assert np.isfinite(a).all(), f"{what}: unwritten {name}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--force", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda:0")

    def want(name):
        path = os.path.join(args.out, name)
        if os.path.exists(path) and not args.force:
            print("kept   ", path)
            return None
        return path

    def save(path, **arrays):
        np.savez_compressed(path, **arrays)
        print("written", path, os.path.getsize(path), "bytes")

    for k, d, world in FE_SHAPES:
        path = want(f"mstep_tail_fe_k{k}_d{d}_w{world}.npz")
        if path is None:
            continue
        packed, avgvar = fe_inputs(k, d, world)
        res = run_fe(packed, avgvar, world, d, True, dev)
        all_finite(res, path)
        bare = run_fe(packed, avgvar, world, d, False, dev)
        for name, a in bare.items():
            assert np.array_equal(a, res[name]), f"{name}: mfac32 changes it"
        if (k, d) in PERK:
            perk = run_perk(res["R"], res["means"], res["pi"], dev)
            all_finite(perk, path)
            res.update(perk)
        save(path, packed=packed, avgvar=avgvar, **res)

    path = want("mstep_tail_reduce.npz")
    if path is not None:
        res = run_reduce(dev)
        all_finite(res, path)
        save(path, **res)

    for d, n in DEAD_SHAPES:
        path = want(f"estep_lds2_deadrows_k{DEAD_K}_d{d}_n{n}.npz")
        if path is None:
            continue
        _, z, mfac, _, add = fam.inputs(DEAD_K, d, n, dev)
        out = fam.run("estep_fused_lds2", z, mfac, add)
        save(path, add=add.cpu().numpy(), z=fam.bits(z), mfac=fam.bits(mfac),
             **out)


if __name__ == "__main__":
    main()
