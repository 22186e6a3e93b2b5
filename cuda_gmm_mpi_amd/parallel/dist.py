"""Distributed backend: one process per GPU, torch.distributed over RCCL.

Replaces the reference's 2-level MPI+OpenMP hierarchy with a
flat world: on ROCm the "nccl" backend IS RCCL and collectives run over
xGMI on device buffers — no host staging, no per-stage D2H/H2D round trips
(deletes the traffic inventory of SURVEY §2.3 entirely).

CPU test runs use the gloo backend (world_size > 1 works without GPUs).
"""
from __future__ import annotations

import datetime
import os

import torch
import torch.distributed as dist


def env_world() -> tuple[int, int, int]:
    """(rank, local_rank, world_size) from torchrun-style env vars."""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    return rank, local_rank, world


def init_process_group(backend: str | None = None,
                       timeout_s: float = 600.0,
                       force: bool = False) -> tuple[int, int, int]:
    """Initialize torch.distributed from the environment.

    A bare world-1 run (no launcher) skips initialization; under a
    launcher (WORLD_SIZE set, e.g. torchrun --nproc-per-node 1) or with
    ``force=True`` a real 1-rank communicator IS created, so RCCL init +
    device-buffer collectives + graph capture execute even on a 1-GPU box
    (world=1 communicator replaces the reference's untested
    MPI path).

    Returns (rank, local_rank, world_size).
    """
    rank, local_rank, world = env_world()
    if world == 1 and "WORLD_SIZE" not in os.environ and not force:
        return rank, local_rank, world
    if backend is None:
        # device-specific backends: RCCL for device buffers, gloo for the
        # CPU-tensor control-plane collectives (outfile/read flags,
        # distribute_input shards + stats). An nccl-only group would raise
        # "no backend for device type cpu" on every multi-rank GPU run.
        backend = ("cpu:gloo,cuda:nccl" if torch.cuda.is_available()
                   else "gloo")
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        # fail fast on collective errors/hangs (the reference
        # aborts on any MPI/CUDA failure; RCCL equivalent is async error
        # handling — a stuck collective aborts after `timeout_s` instead
        # of hanging the job)
        os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
        dist.init_process_group(
            backend=backend, rank=rank, world_size=world,
            timeout=datetime.timedelta(seconds=timeout_s),
        )
    if backend == "nccl":
        torch.cuda.set_device(local_rank)
    return rank, local_rank, world


def is_dist() -> bool:
    return dist.is_available() and dist.is_initialized()


def world_size() -> int:
    return dist.get_world_size() if is_dist() else 1


def rank() -> int:
    return dist.get_rank() if is_dist() else 0


def barrier() -> None:
    if is_dist():
        dist.barrier()


def all_reduce_(t: torch.Tensor) -> torch.Tensor:
    """In-place sum all-reduce on a device buffer (one RCCL call)."""
    if is_dist():
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


def broadcast_(t: torch.Tensor, src: int = 0) -> torch.Tensor:
    if is_dist():
        dist.broadcast(t, src=src)
    return t


def shard_bounds(num_events: int, world: int, r: int) -> tuple[int, int]:
    """Event shard [start, stop) for rank r.

    Correct remainder handling (fixes SURVEY §2.6 #4: the reference assigns
    the remainder via the MPI rank instead of the global GPU index): the
    last rank takes the remainder, every rank's slice is derived from the
    same events_per_gpu so the union covers [0, N) exactly.
    """
    per = num_events // world
    start = per * r
    stop = num_events if r == world - 1 else per * (r + 1)
    return start, stop


def destroy() -> None:
    if is_dist():
        dist.destroy_process_group()


def distribute_input(data: torch.Tensor | None, num_clusters: int,
                     seed_fn=None, seed_info: dict | None = None):
    """Rank-0-read input distribution (reference: MPI_Bcast of the whole
    dataset, gaussian.cu:193-200 — here each rank receives only its SHARD
    via point-to-point sends, sized for N >> full-replication).

    Rank 0 passes the full [N, D] float32 tensor; other ranks pass None.
    Returns (shard, n_total, mean, var, seed_means): the per-rank event
    shard plus the global seeding statistics, computed on rank 0 from the
    full data with exactly the same code as the shared-filesystem path
    (engine.build_engine) so both paths produce identical results.

    ``seed_fn(data) -> (means [K, D], rows [K])`` replaces the strided seeds
    (engine.seed_full_data under the run's config: the data-dependent
    seeding); rank 0 calls it on the full data before the stats broadcast.
    A ``seed_info`` dict receives the broadcast rows under "indices".
    """
    from ..models.seed import seed_indices_strided

    if seed_fn is None:
        def seed_fn(full):
            idx = seed_indices_strided(int(full.shape[0]), num_clusters)
            return full[idx].to(torch.float32), idx

    w, r = world_size(), rank()
    if w == 1:
        n, d = data.shape
        mean = data.double().mean(dim=0).float()
        var = (data.double().pow(2).mean(dim=0)
               - data.double().mean(dim=0).pow(2)).float()
        seed_means, seed_idx = seed_fn(data)
        if seed_info is not None:
            seed_info["indices"] = seed_idx
        return data, n, mean, var, seed_means

    if r == 0:
        if data is None or data.dim() != 2:
            raise ValueError("rank 0 must provide the full [N, D] data")
        shape = torch.tensor(list(data.shape), dtype=torch.long)
    else:
        shape = torch.zeros(2, dtype=torch.long)
    broadcast_(shape)
    n, d = int(shape[0]), int(shape[1])

    k = num_clusters
    stats = torch.zeros(2 * d + k * d, dtype=torch.float32)
    seed_idx = torch.zeros(k, dtype=torch.long)
    if r == 0:
        dmean = data.double().mean(dim=0)
        dvar = data.double().pow(2).mean(dim=0) - dmean * dmean
        stats[:d] = dmean.float()
        stats[d:2 * d] = dvar.float()
        seed_means, seed_idx = seed_fn(data)
        stats[2 * d:] = seed_means.reshape(-1)
    broadcast_(stats)
    if seed_info is not None:
        broadcast_(seed_idx)
        seed_info["indices"] = seed_idx
    mean, var = stats[:d], stats[d:2 * d]
    seed_means = stats[2 * d:].reshape(k, d)

    s, e = shard_bounds(n, w, r)
    if r == 0:
        shard = data[s:e].contiguous()
        reqs = []
        for dst in range(1, w):
            ds_, de_ = shard_bounds(n, w, dst)
            reqs.append(dist.isend(data[ds_:de_].contiguous(), dst=dst))
        for rq in reqs:
            rq.wait()
    else:
        shard = torch.empty(e - s, d, dtype=torch.float32)
        dist.recv(shard, src=0)
    return shard, n, mean, var, seed_means
