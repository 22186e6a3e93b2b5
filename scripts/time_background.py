#!/usr/bin/env python3
"""Time what the uniform background component costs an EM step.

One process, hipEvent timing, warm-up first, the sides alternated within
every repetition (the scheme of time_weights.py). At N x D x K (default:
the flagship 1M x 24 x 64, bf16 E-step + bf16x3 moments as in bench.py,
with every 20th row replaced by uniform noise so that pi0 stays live):

  (a) background_lse alone (no likelihood partials), background_lse with
      the likelihood plus background_update, and event_weight_lse as the
      yardstick of the same memory traffic
  (b) one graph-replayed em_iteration(k, need_lik=False) of four engines on
      the same data:
        lds          unweighted, the default small-K LDS path
        lse          unweighted, use_lds_estep = False (what a background
                     fit runs, minus the background)
        background   lse path + background, switched on
        bg_weighted  the same with weights in {0, 0.5, 1, 2.5}

background - lse is the cost of the background; lse - lds is the cost of
leaving the LDS fast path. Writes one JSON document.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cuda_gmm_mpi_amd.engine import build_engine  # noqa: E402
from cuda_gmm_mpi_amd.ops import functional as F  # noqa: E402
from cuda_gmm_mpi_amd.utils.config import GmmConfig  # noqa: E402
from cuda_gmm_mpi_amd.utils.synthetic import make_bench_data  # noqa: E402


def stats(ms):
    a = np.asarray(ms, dtype=np.float64) * 1e3
    return {"min_us": float(a.min()), "median_us": float(np.median(a)),
            "max_us": float(a.max()), "reps": int(a.size)}


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=24)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU"
    assert args.reps >= 20, "at least 20 timed repetitions"
    n, d, k = args.n, args.d, args.k

    data = make_bench_data(n, d, k)
    rng = np.random.default_rng(0)
    s = rng.choice(np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=n)
    # every 20th row becomes uniform noise over the bounding box (for all
    # four engines alike): on clean blobs pi0 decays to the fixed point 0
    # and the kernel would be timed on its b = -inf branch
    noise = np.arange(0, n, 20)
    lo, hi = data.min(axis=0), data.max(axis=0)
    data[noise] = rng.uniform(lo, hi, (noise.size, d)).astype(np.float32)
    kw = dict(num_clusters=k, target_num_clusters=k, estep_dtype="bf16",
              mstep_precision="bf16x3")
    cfg = GmmConfig(**kw)
    cfg_bg = GmmConfig(background=True, background_warmup=args.warmup, **kw)
    engines = {
        "lds": build_engine(data, cfg, device="cuda"),
        "lse": build_engine(data, cfg, device="cuda"),
        "background": build_engine(data, cfg_bg, device="cuda"),
        "bg_weighted": build_engine(data, cfg_bg, device="cuda", weights=s),
    }
    engines["lse"].use_lds_estep = False
    paths = {name: {"use_lds_estep": bool(e.use_lds_estep),
                    "use_fused_estep": bool(e.use_fused_estep)}
             for name, e in engines.items()}
    for e in engines.values():
        e._estep(k, need_lik=False)
        # the first call captures the graph; the background switches on
        # after `warmup` plain iterations and then runs a few more
        for _ in range(args.warmup + 4):
            e._em_step(k, need_lik=False)
    torch.cuda.synchronize()
    graphed = {name: bool(e._graphs.get((k, False)))
               for name, e in engines.items()}
    switched = {name: bool(e._bg_on) for name, e in engines.items()}
    pi0 = {name: e.background_pi for name, e in engines.items()}

    eb = engines["background"]
    ew = engines["bg_weighted"]
    out_buf = torch.empty_like(eb._lse)
    part = F.background_partial(n, "cuda")
    bg = eb._bg.clone()
    lik = torch.empty(1, device="cuda")

    def lse_and_update():
        F.background_lse(eb._lse, bg, None, None, out_buf, part,
                         need_lik=True, lik_out=lik)
        F.background_update(part[0], float(n), eb.bg_log_volume, bg)

    kern = {
        "background_lse": lambda: F.background_lse(
            eb._lse, eb._bg, None, None, out_buf, part, need_lik=False),
        "background_lse_weighted": lambda: F.background_lse(
            ew._lse, ew._bg, ew.s, ew._lns, out_buf, part, lse_b=ew._lse_b,
            need_lik=False),
        "background_lse_lik_update": lse_and_update,
        "event_weight_lse": lambda: F.event_weight_lse(
            ew._lse, ew.s, ew._lns, out_buf, False),
    }
    for fn in kern.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()

    t = {name: [] for name in list(engines) + list(kern)}
    for _ in range(args.reps):
        evs = {}
        for name, e in engines.items():
            evs[name] = timed(lambda e=e: e.em_iteration(k, need_lik=False))
        for name, fn in kern.items():
            evs[name] = timed(fn)
        torch.cuda.synchronize()
        for name, (a, b) in evs.items():
            t[name].append(a.elapsed_time(b))

    res = {name: stats(v) for name, v in t.items()}
    med = {name: r["median_us"] for name, r in res.items()}
    out = {"shape": {"N": n, "D": d, "K": k},
           "device": torch.cuda.get_device_name(0),
           "paths": paths, "graph_replay": graphed,
           "background_on": switched, "background_pi": pi0, "times": res,
           "background_cost_us": med["background"] - med["lse"],
           "background_weighted_cost_us": med["bg_weighted"] - med["lse"],
           "leaving_lds_cost_us": med["lse"] - med["lds"]}
    text = json.dumps(out, indent=2)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
