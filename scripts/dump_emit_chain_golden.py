#!/usr/bin/env python3
"""Pin the factor chain of emit_mfac (Cholesky of R, triangular inverse) at
the sizes where its D <= 32 form changes shape, as fixtures under
tests/golden/.

  emit_chain_fe_k{K}_d{D}_w{W}.npz   mstep_finalize_emit, inputs and every
      output, as dump_mstep_tail_golden.py lays them out (fe_inputs: with
      K = 3 the N = 0 and N = 0.75 rows are in). For the shapes in PERK also
      lu_* (F.constants) and ef_* (emit_factors) on that R / means / pi.
  emit_chain_clamp_d{D}.npz          emit_factors on a hand-built R that is
      not positive definite: the identity with R[1][0] = R[0][1] = 1.0001.
      1 - 1.0001^2 < 0, so the second pivot is the 1e-8 * diag0 clamp.

tests/test_gpu_emit_chain_golden.py asserts np.array_equal against them, so
run this on the build whose behaviour is to be pinned (the parent of a
change), never on the code under test. Existing files are not rewritten
unless --force is given.

usage: python scripts/dump_emit_chain_golden.py [--out DIR] [--force]
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
import dump_mstep_tail_golden as tail  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

# (K, D, world): one chain step; the first unfused eight of the inverse; the
# head length (j - i) & 7 wrapping twice; the last D of the register form and
# the first D of the general one
FE_SHAPES = [(3, 2, 1), (3, 9, 1), (3, 17, 1), (3, 32, 2), (3, 33, 1)]
PERK = [(3, 9), (3, 32)]
CLAMP_D = [9, 33]


def clamp_inputs(d):
    """R [1, D, D], means [1, D], pi [1]: see the module docstring."""
    r = np.eye(d, dtype=np.float32)
    r[1, 0] = r[0, 1] = np.float32(1.0001)
    means = ((np.arange(d, dtype=np.float32) - 3.0) * 0.25).astype(np.float32)
    return r[None], means[None], np.ones(1, dtype=np.float32)


def run_emit_factors(r, means, pi, with32, dev):
    k, d, _ = r.shape
    _, rows, cols = F.mfac_shape(d)
    rt, mt, pt = (torch.from_numpy(a).to(dev) for a in (r, means, pi))
    mfac = torch.full((k, 2, rows, cols), float("nan"), dtype=torch.bfloat16,
                      device=dev)
    mfac32 = (tail.nans(dev, k, rows, cols) if with32
              else torch.empty(0, dtype=torch.float32, device=dev))
    const, add = tail.nans(dev, k), tail.nans(dev, k)
    hip_ext().emit_factors(rt, mt, mfac, mfac32, pt, const, add)
    torch.cuda.synchronize()
    res = {"constant": const.cpu().numpy(), "add": add.cpu().numpy(),
           "mfac": fam.bits(mfac)}
    if with32:
        res["mfac32"] = mfac32.cpu().numpy()
    return res


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
        path = want(f"emit_chain_fe_k{k}_d{d}_w{world}.npz")
        if path is None:
            continue
        packed, avgvar = tail.fe_inputs(k, d, world)
        res = tail.run_fe(packed, avgvar, world, d, True, dev)
        tail.all_finite(res, path)
        bare = tail.run_fe(packed, avgvar, world, d, False, dev)
        for name, a in bare.items():
            assert np.array_equal(a, res[name]), f"{name}: mfac32 changes it"
        if (k, d) in PERK:
            perk = tail.run_perk(res["R"], res["means"], res["pi"], dev)
            tail.all_finite(perk, path)
            res.update(perk)
        save(path, packed=packed, avgvar=avgvar, **res)

    for d in CLAMP_D:
        path = want(f"emit_chain_clamp_d{d}.npz")
        if path is None:
            continue
        r, means, pi = clamp_inputs(d)
        res = run_emit_factors(r, means, pi, True, dev)
        tail.all_finite(res, path)
        bare = run_emit_factors(r, means, pi, False, dev)
        for name, a in bare.items():
            assert np.array_equal(a, res[name]), f"{name}: mfac32 changes it"
        save(path, R=r, means=means, pi=pi, **res)


if __name__ == "__main__":
    main()
