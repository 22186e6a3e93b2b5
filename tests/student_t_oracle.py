"""Float64 numpy oracle of the Student-t mixture components: the contracts
of the two t kernels / their CPU twins, a float64 t-EM loop in the
parameter-expanded form (with per-event weights), the Gaussian EM next to
it, and the three-blob t3 dataset the engine tests fit.

nu > 0 is fixed. With q the squared Mahalanobis distance, D the dimension
and delta(nu, D) = lgamma((nu + D)/2) - lgamma(nu/2) - D/2 ln(nu/2),

    ln t_c(x) = constant_c + delta - (nu + D)/2 ln(1 + q/nu)
    tau_ce  ∝ pi_c t_c(x_e),   u_ce = (nu + D) / (nu + q_ce)
    M-step on w' = s tau u:  mu = sum w' x / sum w',
                             R = sum w' (x - mu)(x - mu)^T / sum w'
    pi_c = sum_e s_e tau_ce / sum_c (...),  ln L = sum_e s_e lse_t_e

where constant_c is the Gaussian normaliser -D/2 ln 2 pi - 1/2 ln|R_c|.

numpy only.
"""
import math

import numpy as np

INF = float("inf")


# ---------------------------------------------------------------- contract
def delta(nu, d):
    nu = float(nu)
    return (math.lgamma(0.5 * (nu + d)) - math.lgamma(0.5 * nu)
            - 0.5 * d * math.log(0.5 * nu))


def student_t_lse(logw, add, nu, d, s=None, train=True):
    """The kernel's contract on Gaussian log-weights logw [K, N] =
    add_c - q/2 (any float arrays; computed in float64).

    Returns a dict: q, lt = add_c + delta - (nu + D)/2 log1p(q/nu), lnu =
    ln((nu + D)/(nu + q)), lse_t = logsumexp_c lt (-inf where all lt are),
    out (lt + lnu in train mode, lt in posterior mode) and, in train mode,
    lse_m (lse_t, or lse_t - ln s with +inf where s == 0), tau_s [K, N] =
    s exp(lt - lse_t) (exact zeros for s == 0 and for lse_t = -inf), n_c =
    its row sums and lik = sum s lse_t over the events with s > 0."""
    logw = np.asarray(logw, dtype=np.float64)
    add = np.asarray(add, dtype=np.float64)[:, None]
    nu = float(nu)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.maximum(0.0, 2.0 * (add - logw))
        lt = add + delta(nu, d) - 0.5 * (nu + d) * np.log1p(q / nu)
        lnu = np.log((nu + d) / (nu + q))
        m = lt.max(axis=0)
        dead = m == -INF
        ms = np.where(dead, 0.0, m)
        lse_t = np.where(dead, -INF, ms + np.log(np.exp(lt - ms).sum(axis=0)))
        res = {"q": q, "lt": lt, "lnu": lnu, "lse_t": lse_t}
        if not train:
            res["out"] = lt
            return res
        res["out"] = lt + lnu
        tau = np.where(dead[None, :], 0.0,
                       np.exp(lt - np.where(dead, 0.0, lse_t)))
    n = logw.shape[1]
    sw = np.ones(n) if s is None else np.asarray(s, dtype=np.float64)
    live = sw > 0
    lse_m = np.full(n, INF)
    lse_m[live] = lse_t[live] - np.log(sw[live])
    tau_s = np.where(live[None, :], tau * sw[None, :], 0.0)
    res.update(lse_m=lse_m, tau_s=tau_s, n_c=tau_s.sum(axis=1),
               lik=float((sw[live] * lse_t[live]).sum()))
    return res


def student_t_pi(n_c, constant=None):
    """(N, pi, add): N = n_c, pi = n_c / sum n_c with 1e-10 where
    n_c < 0.5, add = constant + ln pi (None without constant)."""
    n_c = np.asarray(n_c, dtype=np.float64)
    pi = np.where(n_c < 0.5, 1e-10, n_c / n_c.sum())
    add = None if constant is None else (
        np.asarray(constant, dtype=np.float64) + np.log(pi))
    return n_c.copy(), pi, add


# ----------------------------------------------------------------- dataset
T3_CENTRES = np.array([[0, 0, 0, 0], [8, 0, 0, 0], [0, 8, 0, 0]], float)


def t3_blobs(seed=5, d=4, per=400, nu_true=3.0):
    """Three D = 4 blobs of `per` events each, unit scale matrix, t3 tails
    (a Gaussian over the root of a chi-square / nu), in blob order: the
    engine's strided seed rows 0, (N - 1)/2, N - 1 fall one in each blob.
    Returns (data fp32 [3 per, d], labels)."""
    rng = np.random.default_rng(seed)
    xs = []
    for c in range(3):
        g = rng.standard_normal((per, d))
        chi = rng.chisquare(nu_true, per) / nu_true
        xs.append(T3_CENTRES[c, :d] + g / np.sqrt(chi)[:, None])
    return (np.ascontiguousarray(np.concatenate(xs), dtype=np.float32),
            np.repeat(np.arange(3), per))


def t_blobs(seed, d, k=4, per=750, nu_true=3.0, sep=8.0):
    """k blobs in d >= k - 1 dimensions with t tails, unit scale matrix, in
    blob order: blob 0 at the origin, blob c at sep along axis c - 1, so the
    strided seed rows fall one in each blob.
    Returns (data fp32 [k per, d], labels)."""
    rng = np.random.default_rng(seed)
    xs = []
    for c in range(k):
        g = rng.standard_normal((per, d))
        chi = rng.chisquare(nu_true, per) / nu_true
        x = g / np.sqrt(chi)[:, None]
        if c:
            x[:, c - 1] += sep
        xs.append(x)
    return (np.ascontiguousarray(np.concatenate(xs), dtype=np.float32),
            np.repeat(np.arange(k), per))


def seed_rows(n, k):
    stride = (n - 1.0) / (k - 1.0) if k > 1 else 0.0
    return [int(c * stride) for c in range(k)]


# ------------------------------------------------------------------ EM loop
def em_fit(data, k, iters, nu=None, s=None, dynamic_range=1e3):
    """Float64 EM from the engine's seeds (strided rows of the events with
    s > 0 as means, R = I, pi = 1/K) with the engine's finalize rule that
    matters on healthy clusters, R = (S - N mu mu^T + avgvar I) / N, avgvar =
    mean per-dimension variance / dynamic_range, N the sum of the M-step's
    weights. nu = None: Gaussian EM (w' = s tau). Otherwise the t-EM in the
    parameter-expanded form (w' = s tau u), pi and N from s tau. Schedule:
    an E-step, then `iters` times (M-step, E-step).

    Returns a dict: means, R, N (= sum s tau), pi, liks (iters + 1 values),
    lik, post (tau [K, n] of the last E-step), ratio (sum s tau u /
    sum s tau per cluster at the last E-step)."""
    x = np.asarray(data, dtype=np.float64)
    n, d = x.shape
    sw = np.ones(n) if s is None else np.asarray(s, dtype=np.float64)
    live = sw > 0
    n_total = float(sw.sum())
    mean = (x * sw[:, None]).sum(axis=0) / n_total
    var = (x * x * sw[:, None]).sum(axis=0) / n_total - mean * mean
    avgvar = var.mean() / dynamic_range
    xs = x[live]
    means = xs[seed_rows(xs.shape[0], k)].copy()
    cov = np.stack([np.eye(d)] * k)
    pi = np.full(k, 1.0 / k)

    def estep():
        q = np.empty((k, n))
        const = np.empty(k)
        for c in range(k):
            diff = x - means[c]
            q[c] = (diff * np.linalg.solve(cov[c], diff.T).T).sum(axis=1)
            const[c] = (-0.5 * d * np.log(2.0 * np.pi)
                        - 0.5 * np.linalg.slogdet(cov[c])[1])
        if nu is None:
            lt = const[:, None] + np.log(pi)[:, None] - 0.5 * q
            u = np.ones_like(q)
        else:
            lt = (const[:, None] + np.log(pi)[:, None] + delta(nu, d)
                  - 0.5 * (nu + d) * np.log1p(q / nu))
            u = (nu + d) / (nu + q)
        m = lt.max(axis=0)
        lse = m + np.log(np.exp(lt - m).sum(axis=0))
        return np.exp(lt - lse), u, float((sw[live] * lse[live]).sum())

    tau, u, lik = estep()
    liks = [lik]
    for _ in range(iters):
        w = tau * u * sw
        nw = w.sum(axis=1)
        means = (w @ x) / nw[:, None]
        for c in range(k):
            sc = (x * w[c][:, None]).T @ x
            cov[c] = (sc - nw[c] * np.outer(means[c], means[c])
                      + avgvar * np.eye(d)) / nw[c]
        nc = (tau * sw).sum(axis=1)
        pi = nc / nc.sum()
        tau, u, lik = estep()
        liks.append(lik)
    nc = (tau * sw).sum(axis=1)
    return {"means": means, "R": cov, "N": nc, "pi": pi,
            "liks": np.array(liks), "lik": lik, "post": tau,
            "ratio": (tau * u * sw).sum(axis=1) / nc}
