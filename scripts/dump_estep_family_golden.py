#!/usr/bin/env python3
"""Pin the raw outputs of the five small-D fused E-step kernels as fixtures.

For every kernel and shape below, writes one ``.npz`` holding the inputs
the kernel reads and what it wrote into NaN-filled outputs:

  x (f32 kernels) or z (bf16 kernels, as uint16 bits)   [D, N]
  mfac32 [K,32,32] f32  or  mfac [K,2,32,32] as uint16 bits
  add [K], w [K,N], partial [nblk], and lse [N] where the kernel has one

tests/test_gpu_estep_family_golden.py asserts np.array_equal against them,
so run this on the build whose behaviour is to be pinned (the parent of a
refactor), never on the code under test. Existing files are not rewritten
unless --force is given.

usage: python scripts/dump_estep_family_golden.py [--out DIR] [--force]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.ops.backend import hip_ext  # noqa: E402

# entry point -> (fixture stem, input precision, events per block, has lse)
KERNELS = {
    "estep_fused": ("estep_fused", "bf16", 256, True),
    "estep_fused_f32": ("estep_fused_f32", "f32", 256, True),
    "estep_fused_lds": ("estep_fused_lds", "bf16", 128, False),
    "estep_fused_lds2": ("estep_fused_lds2", "bf16", 128, False),
    "estep_fused_f32_lds": ("estep_f32_lds", "f32", 128, False),
}
SHAPES = [(9, 24, 313), (5, 31, 257), (3, 1, 300)]


def fixture_name(entry, k, d, n):
    return f"{KERNELS[entry][0]}_k{k}_d{d}_n{n}.npz"


def bits(t):
    """bf16 tensor -> uint16 numpy array of its bit patterns."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def inputs(k, d, n, dev):
    rng = np.random.default_rng(100000 * d + 1000 * k + n)
    means = torch.from_numpy(
        rng.standard_normal((k, d)).astype(np.float32) * 2).to(dev)
    rs = []
    for _ in range(k):
        a = rng.standard_normal((d, d))
        rs.append((a @ a.T + d * np.eye(d)).astype(np.float32))
    r = torch.from_numpy(np.stack(rs)).to(dev)
    pi = torch.from_numpy(rng.dirichlet(np.ones(k)).astype(np.float32)).to(dev)
    mfac = torch.empty(k, 2, 32, 32, dtype=torch.bfloat16, device=dev)
    mfac32 = torch.empty(k, 32, 32, dtype=torch.float32, device=dev)
    _, const = F.constants(r, means, False, mfac, mfac32)
    add = (const + torch.log(pi)).contiguous()
    x = torch.from_numpy(
        rng.standard_normal((d, n)).astype(np.float32) * 2).to(dev)
    return x, x.to(torch.bfloat16).contiguous(), mfac, mfac32, add


def run(entry, z, fac, add):
    _, _, tile, has_lse = KERNELS[entry]
    k, n = add.shape[0], z.shape[1]
    nan = float("nan")
    w = torch.full((k, n), nan, dtype=torch.float32, device=z.device)
    partial = torch.full(((n + tile - 1) // tile,), nan, dtype=torch.float32,
                         device=z.device)
    out = {"w": w, "partial": partial}
    if has_lse:
        out["lse"] = torch.full((n,), nan, dtype=torch.float32,
                                device=z.device)
        getattr(hip_ext(), entry)(z, fac, add, w, out["lse"], partial)
    else:
        getattr(hip_ext(), entry)(z, fac, add, w, partial)
    torch.cuda.synchronize()
    for name, t in out.items():
        assert bool(torch.isfinite(t).all()), f"{entry}: unwritten {name}"
    return {name: t.cpu().numpy() for name, t in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--force", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda:0")
    for k, d, n in SHAPES:
        x, z, mfac, mfac32, add = inputs(k, d, n, dev)
        for entry, (_, prec, _, _) in KERNELS.items():
            path = os.path.join(args.out, fixture_name(entry, k, d, n))
            if os.path.exists(path) and not args.force:
                print("kept   ", path)
                continue
            if prec == "bf16":
                arrays = {"z": bits(z), "mfac": bits(mfac)}
                out = run(entry, z, mfac, add)
            else:
                arrays = {"x": x.cpu().numpy(),
                          "mfac32": mfac32.cpu().numpy()}
                out = run(entry, x, mfac32, add)
            np.savez(path, add=add.cpu().numpy(), **arrays, **out)
            print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
