"""``python -m cuda_gmm_mpi_amd.classify MODEL INFILE OUTSTEM`` — score a
data file with a saved model.

MODEL is a .npz written by ``gmm ... --save-model`` or, chosen by its
suffix, a .summary file (lossy: %.3f parameters). Writes OUTSTEM.labels,
one line per event: ``label,max posterior,log-probability`` as %d,%f,%f.
A model with a uniform background labels the events it assigns to it -1.
A model with Student-t components (``gmm --student-t NU``) is scored with
its t densities.

Exit codes: 0 ok, 1 bad arguments, 2 unreadable INFILE (as ``gmm``),
5 unreadable MODEL or a model / data dimension mismatch.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import numpy as np
import torch

from .models.model import GmmModel
from .utils import io as gio


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="python -m cuda_gmm_mpi_amd.classify",
        description="Assign the events of a data file to the clusters of a "
                    "saved model")
    p.add_argument("model", help="model .npz (gmm --save-model) or a "
                                 ".summary file")
    p.add_argument("infile", help="FCS data file (.bin binary or CSV)")
    p.add_argument("outstem", help="output file stem")
    p.add_argument("--device", default=None, choices=["cpu", "cuda"],
                   help="cpu | cuda (default: cuda when available)")
    p.add_argument("--estep-dtype", choices=["fp32", "bf16"], default="fp32")
    p.add_argument("--chunk-events", type=int, default=1 << 22,
                   help="events per device chunk")
    p.add_argument("--memberships", action="store_true",
                   help="also write OUTSTEM.results (full posteriors)")
    p.add_argument("--metrics-out", default=None,
                   help="write machine-readable run metrics (JSON) here")
    return p


def write_labels(path: str, pred, chunk: int = 65536) -> None:
    with open(path, "w") as f:
        for s in range(0, pred.labels.shape[0], chunk):
            e = s + chunk
            f.write("".join(
                "%d,%f,%f\n" % row
                for row in zip(pred.labels[s:e].tolist(),
                               pred.max_posterior[s:e].tolist(),
                               pred.log_prob[s:e].tolist())))


def main(argv=None) -> int:
    try:
        args = make_parser().parse_args(argv)
    except SystemExit as e:
        return 0 if e.code == 0 else 1
    if args.chunk_events < 1:
        print("--chunk-events must be >= 1\n")
        return 1
    try:
        if args.model.endswith(".summary"):
            model = GmmModel.from_summary(args.model)
        else:
            model = GmmModel.load(args.model)
    except (OSError, ValueError) as e:
        print(f"Invalid model. ({e})\n")
        return 5
    try:
        data = gio.read_data(args.infile)
    except (OSError, ValueError) as e:
        print(f"Invalid infile. ({e})\n")
        return 2
    if data.shape[1] != model.num_dimensions:
        print(f"Invalid model. (data has D={data.shape[1]}, the model has "
              f"D={model.num_dimensions})\n")
        return 5
    if not np.isfinite(data).all():
        bad = int((~np.isfinite(data)).sum())
        print(f"WARNING: input contains {bad} non-finite values; "
              "results will be degenerate", file=sys.stderr)
    device = args.device
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"

    t_start = time.perf_counter()
    pred = model.predict(data, device=device, estep_dtype=args.estep_dtype,
                         chunk_events=args.chunk_events)
    write_labels(args.outstem + ".labels", pred)
    if args.memberships:
        w = model.posteriors(data, device=device,
                             estep_dtype=args.estep_dtype,
                             chunk_events=args.chunk_events)
        gio.write_results(args.outstem + ".results", data, w)
    elapsed = time.perf_counter() - t_start
    if args.metrics_out:
        with open(args.metrics_out, "w") as f:
            json.dump({
                "N": int(data.shape[0]),
                "K": model.num_clusters,
                "D": model.num_dimensions,
                "log_likelihood": pred.log_likelihood,
                "counts": pred.counts.tolist(),
                "background_count": pred.background_count,
                "student_t_nu": model.student_t_nu,
                "device": device,
                "seconds": elapsed,
            }, f, indent=2)
    return 0


if __name__ == "__main__":
    sys.exit(main())
