"""Deterministic cluster seeding.

Reference behavior: the GPU seed kernel
(gaussian_kernel.cu:269-328) computes avgvar on the master GPU's shard and
sets R=I, pi=1/K, then the host ``seed_clusters`` (gaussian.cu:108-123)
overwrites means and N from evenly-strided events of the FULL dataset, and
the result is broadcast. What survives the overwrite: R=I, pi=1/K, avgvar,
and the host means/N.

MI355X-native version: deterministic and GPU-count independent — the
strided means come from the full dataset (exactly the host formula) and
avgvar is computed from full-data sums reduced across shards, so 1-GPU and
8-GPU runs seed identically.

Beyond the reference: ``seed_method="kmeans++"`` replaces the strided rows
with a greedy k-means++ (D^2-sampling) draw over the full dataset, which does
not depend on the row order of the file. ``seed_means_kmeanspp`` is its
float64 host implementation; everything else the seed state sets (R, pi, N,
avgvar) stays as ``seed_state`` sets it.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .state import GmmState


def seed_means_host(data_by_event: torch.Tensor, num_clusters: int) -> torch.Tensor:
    """Evenly-strided event means (host seed_clusters, gaussian.cu:108-123).

    means[c] = data[(int)(c * seed)] with seed = (N-1)/(K-1).
    data_by_event: [N, D].
    """
    idx = seed_indices_strided(data_by_event.shape[0], num_clusters)
    return data_by_event[idx].to(torch.float32)


def seed_indices_strided(num_events: int, num_clusters: int) -> torch.Tensor:
    """Rows of the evenly-strided seeds: (int)(c * (N-1)/(K-1)), [K] int64."""
    if num_clusters > 1:
        seed = (num_events - 1.0) / (num_clusters - 1.0)
    else:
        seed = 0.0
    return torch.tensor(
        [int(c * seed) for c in range(num_clusters)], dtype=torch.long
    )


# uniforms per round; 2 + floor(ln K) <= 8 for every K <= MAX_CLUSTERS (512)
KMEANSPP_MAX_CANDIDATES = 8


def kmeanspp_num_candidates(num_clusters: int) -> int:
    """Candidates per round of greedy k-means++: L = 2 + floor(ln K)."""
    return 2 + int(math.floor(math.log(num_clusters)))


def kmeanspp_uniforms(num_clusters: int, seed_rng: int) -> np.ndarray:
    """The uniforms of a seeding, float64 [K, 8]: round 0 uses [0, 0], round
    t >= 1 uses [t, 0:L]. Drawn once on the host for CPU and GPU alike."""
    return np.random.default_rng(seed_rng).random(
        (num_clusters, KMEANSPP_MAX_CANDIDATES))


def kmeanspp_pick(p: np.ndarray, u: float) -> int:
    """Smallest e with cumsum(p)[e] > u * sum(p), clamped to N-1; the
    cumulative sum runs in event order in float64. An event with p == 0
    repeats its predecessor's cumulative value and is never returned."""
    cum = np.cumsum(p, dtype=np.float64)
    e = int(np.searchsorted(cum, u * cum[-1], side="right"))
    return min(e, p.shape[0] - 1)


def seed_means_kmeanspp(data, k: int, seed_rng: int, weights=None
                        ) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """Greedy k-means++ seeds of the full dataset, in float64 on the host:
    the CPU device's seeding and the oracle of the GPU kernels.

    data [N, D] (event-major, as read from the file); ``weights`` [N] are
    per-event weights s >= 0 (None: every event counts once). Round 0 picks
    row i0 = pick(s, U[0, 0]) and sets m_e = |x_e - x_i0|^2. Round t draws
    L = 2 + floor(ln K) candidates c_l = pick(s * m, U[t, l]) (pick(s, .) when
    s * m sums to zero: fewer distinct rows than clusters), keeps the lowest
    l that minimises pot_l = sum_e s_e min(m_e, |x_e - x_c_l|^2) and lowers m
    to that minimum. Distances are sums of squared differences (no
    |x|^2 - 2 x.c + |c|^2 expansion: it cancels at FCS-scale data).

    Returns (means fp32 [K, D] = data[indices], indices int64 [K] in pick
    order, trace) with trace = {"candidates": int64 [K, L] (-1 in the unused
    slots of round 0), "winner": int64 [K] winning slot, "potentials":
    float64 [K, L] (NaN where unused)}.
    """
    x32 = (data.detach().cpu().numpy() if isinstance(data, torch.Tensor)
           else np.asarray(data))
    x = np.ascontiguousarray(x32, dtype=np.float64)
    n = x.shape[0]
    if weights is None:
        s = np.ones(n, dtype=np.float64)
    else:
        s = (weights.detach().cpu().numpy()
             if isinstance(weights, torch.Tensor) else np.asarray(weights))
        s = s.reshape(-1).astype(np.float64)
    nl = kmeanspp_num_candidates(k)
    u = kmeanspp_uniforms(k, seed_rng)

    def dist2(row: int) -> np.ndarray:
        diff = x - x[row]
        return np.einsum("ij,ij->i", diff, diff)

    cands = np.full((k, nl), -1, dtype=np.int64)
    winner = np.zeros(k, dtype=np.int64)
    pots = np.full((k, nl), np.nan)
    indices = np.empty(k, dtype=np.int64)

    i0 = kmeanspp_pick(s, u[0, 0])
    m = dist2(i0)
    cands[0, 0] = indices[0] = i0
    pots[0, 0] = float(np.sum(s * m))
    for t in range(1, k):
        p = s * m
        if float(np.sum(p)) == 0.0:
            p = s
        best = None
        for l in range(nl):
            c = kmeanspp_pick(p, u[t, l])
            dl = np.minimum(m, dist2(c))
            cands[t, l] = c
            pots[t, l] = float(np.sum(s * dl))
            if best is None or pots[t, l] < pots[t, winner[t]]:
                best, winner[t] = dl, l
        m = best
        indices[t] = cands[t, winner[t]]
    idx = torch.from_numpy(indices)
    means = torch.as_tensor(x32)[idx].to(torch.float32)
    trace = {"candidates": torch.from_numpy(cands),
             "winner": torch.from_numpy(winner),
             "potentials": torch.from_numpy(pots)}
    return means, idx, trace


def seed_state(
    state: GmmState,
    seed_means: torch.Tensor,   # [K, D] from seed_means_host on full data
    total_variance_per_dim: torch.Tensor,  # [D] full-data per-dim variance
    num_events_total: int,
    covariance_dynamic_range: float,
) -> None:
    """Populate a GmmState in place with the reference's surviving seed
    values: means (strided events), N = N_total/K (integer division,
    gaussian.cu:118), pi = 1/K, R = I, avgvar = mean(var)/CDR
    (gaussian_kernel.cu:316-326)."""
    k, d = state.num_clusters, state.num_dimensions
    state.means.copy_(seed_means.to(state.means.device))
    state.N.fill_(float(num_events_total // k))
    state.pi.fill_(1.0 / k)
    avgvar = float(total_variance_per_dim.mean()) / covariance_dynamic_range
    state.avgvar.fill_(avgvar)
    eye = torch.eye(d, dtype=torch.float32, device=state.R.device)
    state.R.copy_(eye.expand(k, d, d))
