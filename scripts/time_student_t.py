#!/usr/bin/env python3
"""Time what Student-t components cost an EM step.

One process, hipEvent timing, warm-up first, the sides alternated within
every repetition (the scheme of time_background.py). At N x D x K (default:
the flagship 1M x 24 x 64, bf16 E-step + bf16x3 moments as in bench.py):

  (a) student_t_lse_kernel alone (one launch at the extension, no
      reduction kernels) over the [K, N] log-weight buffer of a fused
      E-step (restored from a copy before every repetition, outside the
      timed region: the kernel rewrites it in place), in train mode with
      and without the likelihood partials, weighted, and in posterior mode;
      the train launch followed by reduce_chunks and reduce_scalar as the
      engine issues it; and estep_lse_kernel over the same buffer as the
      yardstick of one read of it. Train mode reads the buffer twice and
      writes it once, posterior mode reads and writes it once.
  (b) one graph-replayed em_iteration(k, need_lik=False) of four engines on
      the same data:
        lds          Gaussian, the default small-K LDS path
        lse          Gaussian, use_lds_estep = False (what a t fit runs,
                     minus the t pass)
        student_t    lse path + student_t_lse + reduce + student_t_pi
        t_weighted   the same with weights in {0, 0.5, 1, 2.5}

student_t - lse is the cost of the t components; lse - lds is the cost of
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
    ap.add_argument("--nu", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU"
    assert args.reps >= 20, "at least 20 timed repetitions"
    n, d, k, nu = args.n, args.d, args.k, args.nu

    data = make_bench_data(n, d, k)
    s = np.random.default_rng(0).choice(
        np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=n)
    kw = dict(num_clusters=k, target_num_clusters=k, estep_dtype="bf16",
              mstep_precision="bf16x3")
    cfg = GmmConfig(**kw)
    cfg_t = GmmConfig(student_t_nu=nu, **kw)
    engines = {
        "lds": build_engine(data, cfg, device="cuda"),
        "lse": build_engine(data, cfg, device="cuda"),
        "student_t": build_engine(data, cfg_t, device="cuda"),
        "t_weighted": build_engine(data, cfg_t, device="cuda", weights=s),
    }
    engines["lse"].use_lds_estep = False
    paths = {name: {"use_lds_estep": bool(e.use_lds_estep),
                    "use_fused_estep": bool(e.use_fused_estep)}
             for name, e in engines.items()}
    for e in engines.values():
        e._estep(k, need_lik=False)
        for _ in range(args.warmup + 2):   # the first call captures
            e.em_iteration(k, need_lik=False)
    torch.cuda.synchronize()
    graphed = {name: bool(e._graphs.get((k, False)))
               for name, e in engines.items()}

    # (a) the kernel alone, on the Gaussian log-weights of the lse engine
    el = engines["lse"]
    ew = engines["t_weighted"]
    el._estep(k, need_lik=False)
    torch.cuda.synchronize()
    saved = el.w[:k].clone()
    buf = torch.empty_like(saved)
    add = el._add[:k].clone()
    lse_m, lse_t = torch.empty_like(el._lse), torch.empty_like(el._lse)
    n_part, lik_part = F.student_t_partials(n, k, "cuda")
    n_c = torch.empty(k, device="cuda")
    lik = torch.empty(1, device="cuda")
    yard_lse = torch.empty_like(el._lse)

    from cuda_gmm_mpi_amd.ops.backend import hip_ext
    ext = hip_ext()
    empty = buf.new_empty(0)
    delta = F.student_t_delta(nu, d)

    def train(need_lik, weighted=False):
        return lambda: ext.student_t_lse(
            buf, add, ew.s if weighted else empty,
            ew._lns if weighted else empty, lse_m, lse_t, n_part,
            lik_part if need_lik else empty, nu, d, delta, True)

    kern = {
        "student_t_lse_train": train(False),
        "student_t_lse_train_lik": train(True),
        "student_t_lse_train_weighted": train(False, True),
        "student_t_lse_posterior": lambda: ext.student_t_lse(
            buf, add, empty, empty, empty, lse_t, empty, empty, nu, d,
            delta, False),
        "student_t_lse_train_lik_and_reductions": lambda: F.student_t_lse(
            buf, add, nu, d, None, None, lse_m, lse_t, n_part, lik_part,
            n_c, need_lik=True, lik_out=lik),
        "estep_lse": lambda: F.estep_lse(buf, yard_lse, need_lik=False),
    }
    for fn in kern.values():
        for _ in range(args.warmup):
            buf.copy_(saved)
            fn()
    torch.cuda.synchronize()

    t = {name: [] for name in list(engines) + list(kern)}
    for _ in range(args.reps):
        evs = {}
        for name, e in engines.items():
            evs[name] = timed(lambda e=e: e.em_iteration(k, need_lik=False))
        for name, fn in kern.items():
            buf.copy_(saved)          # not timed
            evs[name] = timed(fn)
        torch.cuda.synchronize()
        for name, (a, b) in evs.items():
            t[name].append(a.elapsed_time(b))

    res = {name: stats(v) for name, v in t.items()}
    med = {name: r["median_us"] for name, r in res.items()}
    nbytes = 4.0 * k * n
    out = {"shape": {"N": n, "D": d, "K": k, "nu": nu},
           "device": torch.cuda.get_device_name(0),
           "paths": paths, "graph_replay": graphed, "times": res,
           "logw_buffer_bytes": nbytes,
           # buffer bytes per second, counting every pass a kernel makes
           # over the buffer wherever it is served from: estep_lse 1 read
           # (its second sweep of an event's column hits the cache lines
           # the first brought in), train 2 reads + 1 write, posterior
           # 1 read + 1 write
           "estep_lse_GBps": nbytes / med["estep_lse"] / 1e3,
           "student_t_lse_train_GBps":
               3 * nbytes / med["student_t_lse_train"] / 1e3,
           "student_t_lse_posterior_GBps":
               2 * nbytes / med["student_t_lse_posterior"] / 1e3,
           "train_fraction_of_estep_lse_rate":
               3 * med["estep_lse"] / med["student_t_lse_train"],
           "posterior_fraction_of_estep_lse_rate":
               2 * med["estep_lse"] / med["student_t_lse_posterior"],
           "train_time_over_estep_lse_time":
               med["student_t_lse_train"] / med["estep_lse"],
           "student_t_cost_us": med["student_t"] - med["lse"],
           "student_t_weighted_cost_us": med["t_weighted"] - med["lse"],
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
