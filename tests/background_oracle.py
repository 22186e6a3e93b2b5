"""Float64 numpy oracle of the uniform background component: the contract
of the background kernels / their CPU twins, a float64 EM loop with a
background, and the blobs-plus-noise dataset the engine tests fit.

The mixture is (1 - pi0) * sum_c pi_c N_c(x) + pi0 / V with pi_c normalised
among the Gaussians and V the volume of a box. With the Gaussian-only
per-event lse = ln sum_c pi_c N_c(x) and b = ln(pi0 / (1 - pi0)) - ln V,

    lse_b = logaddexp(lse, b)             ln(p(x) / (1 - pi0))
    r0    = exp(b - lse_b)                background posterior
    ln L  = sum_e lse_b_e + n_total ln(1 - pi0)

numpy only.
"""
import numpy as np

INF = float("inf")


# ---------------------------------------------------------------- contract
def background_lse(lse, b, s=None):
    """(lse_b, lse_m, n0, lik), float64.

    lse_b = max(lse, b) + log1p(exp(-|lse - b|)); both -inf -> -inf;
    b = -inf -> lse itself. r0 = exp(b - lse_b), 0 at b = -inf. lse_m is
    the lse the moments kernels read: lse_b, or lse_b - ln s with weights
    (+inf where s == 0). n0 = sum s r0 and lik = sum s lse_b, events with
    s == 0 skipped, not multiplied."""
    lse = np.asarray(lse, dtype=np.float64)
    b = float(b)
    if b == -INF:
        lse_b = lse.copy()
        r0 = np.zeros_like(lse)
    else:
        hi = np.maximum(lse, b)
        with np.errstate(invalid="ignore"):
            gap = np.abs(lse - b)
        lse_b = hi + np.log1p(np.exp(-gap))
        r0 = np.exp(b - lse_b)
    if s is None:
        return lse_b, lse_b.copy(), float(r0.sum()), float(lse_b.sum())
    s = np.asarray(s, dtype=np.float64)
    live = s > 0
    lse_m = np.full_like(lse_b, INF)
    lse_m[live] = lse_b[live] - np.log(s[live])
    n0 = float((s[live] * r0[live]).sum())
    lik = float((s[live] * lse_b[live]).sum())
    return lse_b, lse_m, n0, lik


def background_update(n0, n_total, ln_v):
    """(pi0, b, lik_add): pi0 = min(n0 / n_total, 1 - 1e-6),
    b = ln pi0 - ln(1 - pi0) - ln V (-inf at pi0 = 0),
    lik_add = n_total ln(1 - pi0)."""
    pi0 = min(float(n0) / float(n_total), 1.0 - 1e-6)
    if pi0 <= 0.0:
        return 0.0, -INF, 0.0
    l1m = np.log1p(-pi0)
    return pi0, float(np.log(pi0) - l1m - ln_v), float(n_total * l1m)


def log_volume(data, s=None):
    x = np.asarray(data, dtype=np.float64)
    if s is not None:
        x = x[np.asarray(s) > 0]
    return float(np.log(x.max(axis=0) - x.min(axis=0)).sum())


# ----------------------------------------------------------------- dataset
def blobs_plus_noise(seed=0, d=20, k=3, per_blob=2000, n_noise=600,
                     scale=100.0, spread=12.0, mix=0.5 / np.sqrt(5.0)):
    """k Gaussian blobs (means uniform in +-spread per dimension, covariance
    A A^T with A = I + mix N(0, 1), mix = 0.5 / sqrt(5) by default) plus
    n_noise events uniform over the blobs' bounding box widened by 5 per
    side, all times `scale`.
    Rows are shuffled, then one event of each blob is swapped into each of
    the k strided seed rows (int)(c (N - 1) / (k - 1)).
    Returns (data fp32 [N, d], labels [N], -1 = noise)."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-spread, spread, (k, d))
    rows, labels = [], []
    for c in range(k):
        a = np.eye(d) + mix * rng.standard_normal((d, d))
        rows.append(means[c] + rng.standard_normal((per_blob, d)) @ a.T)
        labels.append(np.full(per_blob, c))
    blobs = np.concatenate(rows)
    lo, hi = blobs.min(axis=0) - 5.0, blobs.max(axis=0) + 5.0
    rows.append(rng.uniform(lo, hi, (n_noise, d)))
    labels.append(np.full(n_noise, -1))
    data = np.concatenate(rows) * scale
    labels = np.concatenate(labels)
    perm = rng.permutation(data.shape[0])
    data, labels = data[perm], labels[perm]
    n = data.shape[0]
    seeds = seed_rows(n, k)
    for c, p in enumerate(seeds):
        if labels[p] == c:
            continue
        q = next(int(j) for j in np.nonzero(labels == c)[0]
                 if int(j) not in seeds)
        data[[p, q]] = data[[q, p]]
        labels[[p, q]] = labels[[q, p]]
    return np.ascontiguousarray(data, dtype=np.float32), labels


def seed_rows(n, k):
    stride = (n - 1.0) / (k - 1.0) if k > 1 else 0.0
    return [int(c * stride) for c in range(k)]


# ------------------------------------------------------------------ EM loop
def em_fit(data, k, iters, background=True, init=0.01, warmup=5, s=None,
           ln_v=None, dynamic_range=1e3):
    """Float64 EM from the engine's seeds (strided rows as means, R = I,
    pi = 1/K) with the engine's finalize rules that matter on healthy
    clusters: R = (S - N mu mu^T + avgvar I) / N with avgvar = mean
    per-dimension variance / dynamic_range. The schedule is the engine's:
    an E-step, then `iters` times (M-step, background update, E-step); the
    background is switched on at pi0 = init before the iteration that
    follows `warmup` plain ones, by redoing the background pass of the
    current E-step.

    Returns a dict: pi0, n0, means, R, N, pi, lik, post [K + 1, n] (the
    last E-step's posteriors, background last)."""
    x = np.asarray(data, dtype=np.float64)
    n, d = x.shape
    sw = np.ones(n) if s is None else np.asarray(s, dtype=np.float64)
    live = sw > 0
    n_total = float(sw.sum())
    if ln_v is None:
        ln_v = log_volume(x, None if s is None else sw)
    mean = (x * sw[:, None]).sum(axis=0) / n_total
    var = (x * x * sw[:, None]).sum(axis=0) / n_total - mean * mean
    avgvar = var.mean() / dynamic_range
    xs = x[live]
    means = xs[seed_rows(xs.shape[0], k)].copy()
    cov = np.stack([np.eye(d)] * k)
    pi = np.full(k, 1.0 / k)
    pi0, b, lik_add = 0.0, -INF, 0.0

    def gauss_logw():
        out = np.empty((k, n))
        for c in range(k):
            diff = x - means[c]
            sol = np.linalg.solve(cov[c], diff.T).T
            _, logdet = np.linalg.slogdet(cov[c])
            out[c] = (-0.5 * (diff * sol).sum(axis=1)
                      - 0.5 * d * np.log(2.0 * np.pi) - 0.5 * logdet
                      + np.log(pi[c]))
        return out

    def estep():
        logw = gauss_logw()
        m = logw.max(axis=0)
        lse = m + np.log(np.exp(logw - m).sum(axis=0))
        lse_b, _, n0, lik = background_lse(lse, b, None if s is None else sw)
        return logw, lse_b, n0, lik + lik_add

    logw, lse_b, n0, lik = estep()
    on, plain = False, 0
    for _ in range(iters):
        if background and not on and plain >= warmup:
            pi0, b, lik_add = background_update(init * n_total, n_total,
                                                ln_v)
            on = True
            logw, lse_b, n0, lik = estep()
        w = np.exp(logw - lse_b) * sw
        nc = w.sum(axis=1)
        means = (w @ x) / nc[:, None]
        for c in range(k):
            sc = (x * w[c][:, None]).T @ x
            cov[c] = (sc - nc[c] * np.outer(means[c], means[c])
                      + avgvar * np.eye(d)) / nc[c]
        pi = nc / nc.sum()
        if on:
            pi0, b, lik_add = background_update(n0, n_total, ln_v)
        logw, lse_b, n0, lik = estep()
        if not on:
            plain += 1
    r0 = np.exp(b - lse_b) if b != -INF else np.zeros(n)
    post = np.concatenate([np.exp(logw - lse_b), r0[None, :]])
    return {"pi0": pi0, "n0": n0, "means": means, "R": cov, "N": nc,
            "pi": pi, "lik": lik, "post": post, "ln_v": ln_v}
