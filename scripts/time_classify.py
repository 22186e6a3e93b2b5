#!/usr/bin/env python3
"""Time the classify kernels against what scoring costs without them.

One process, hipEvent timing, warm-up first, the sides alternated within
every repetition. Per dtype at N x D x K (default: the flagship 1M x 24 x
64):

  (a) the composition available without the kernel, piece by piece:
      prep   torch centre + transpose (+ bf16 cast) of event-major x
      estep  estep_fused / estep_fused_f32 into a [K, N] buffer
      post   torch max(dim=0) and exp(max - lse)
  (b) estep_classify / estep_classify_f32 alone
  (c) GmmModel.predict end to end from host memory, in events/s

Gate: (b) is faster than the sum of (a) beyond the spread of the
repetitions, i.e. max(b) < min(a sum). Writes one JSON document.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuda_gmm_mpi_amd import GmmModel  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402


def stats(ms):
    a = np.asarray(ms, dtype=np.float64)
    return {"min_ms": float(a.min()), "median_ms": float(np.median(a)),
            "max_ms": float(a.max()), "reps": int(a.size)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=24)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--predict-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU"
    assert args.reps >= 20, "at least 20 timed repetitions"
    dev = torch.device("cuda:0")
    n, d, k = args.n, args.d, args.k
    rng = np.random.default_rng(0)

    means = rng.standard_normal((k, d)).astype(np.float32) * 4
    rs = []
    for _ in range(k):
        a = rng.standard_normal((d, d))
        rs.append((a @ a.T / d + np.eye(d)).astype(np.float32))
    r = np.stack(rs)
    pi = rng.dirichlet(np.full(k, 5.0)).astype(np.float32)
    which = rng.integers(0, k, n)
    data = (means[which] + rng.standard_normal((n, d)).astype(np.float32)
            + 100.0).astype(np.float32)
    model = GmmModel.from_params(means + 100.0, r, pi)

    x = torch.from_numpy(data).to(dev)                    # [N, D]
    center = model.center.to(dev)
    st = model._on(dev)
    out = {"shape": {"N": n, "D": d, "K": k},
           "device": torch.cuda.get_device_name(0), "dtypes": {}}
    ok = True
    for dtype in ("bf16", "fp32"):
        fac, add = F.model_factor_tables(st.means, st.R, st.Rinv,
                                         st.constant, st.pi, False, dtype)
        w = torch.empty(k, n, dtype=torch.float32, device=dev)
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        estep = F.estep_fused if dtype == "bf16" else F.estep_fused_f32

        def prep():
            z = (x - center.unsqueeze(0)).T.contiguous()
            return z.to(torch.bfloat16) if dtype == "bf16" else z

        def post():
            m = w.max(dim=0)
            return m.indices, torch.exp(m.values - lse)

        def classify():
            return F.estep_classify(x, center, fac, add, dtype)

        z = prep()
        for _ in range(args.warmup):
            prep()
            estep(z, fac, add, w, lse, need_lik=False)
            post()
            classify()
        torch.cuda.synchronize()
        t = {"prep": [], "estep": [], "post": [], "sum": [], "classify": []}
        for _ in range(args.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            z = prep()
            ev[1].record()
            estep(z, fac, add, w, lse, need_lik=False)
            ev[2].record()
            post()
            ev[3].record()
            ev[4].record()
            classify()
            ev[5].record()
            torch.cuda.synchronize()
            p, e, q = (ev[i].elapsed_time(ev[i + 1]) for i in range(3))
            t["prep"].append(p)
            t["estep"].append(e)
            t["post"].append(q)
            t["sum"].append(ev[0].elapsed_time(ev[3]))
            t["classify"].append(ev[4].elapsed_time(ev[5]))
        # same answers on the timed inputs
        lab, lse_c, _ = classify()
        same_lse = bool(torch.equal(lse_c, lse))
        same_lab = float((lab.long() == w.max(dim=0).indices).float().mean())
        wall = []
        model.predict(data, device="cuda", estep_dtype=dtype)
        for _ in range(args.predict_reps):
            t0 = time.perf_counter()
            model.predict(data, device="cuda", estep_dtype=dtype)
            wall.append(time.perf_counter() - t0)
        res = {name: stats(v) for name, v in t.items()}
        res["predict_seconds"] = {"min": min(wall),
                                  "median": float(np.median(wall)),
                                  "max": max(wall), "reps": len(wall)}
        res["predict_events_per_s"] = n / float(np.median(wall))
        res["lse_bit_equal_to_estep"] = same_lse
        res["label_share_equal_to_torch_argmax"] = same_lab
        res["gate_classify_faster_than_sum"] = bool(
            res["classify"]["max_ms"] < res["sum"]["min_ms"])
        res["classify_le_estep_alone"] = bool(
            res["classify"]["median_ms"] <= res["estep"]["median_ms"])
        ok = ok and res["gate_classify_faster_than_sum"]
        out["dtypes"][dtype] = res
        print(dtype, json.dumps(res))
    text = json.dumps(out, indent=2)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print("gate:", "holds" if ok else "FAILS")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
