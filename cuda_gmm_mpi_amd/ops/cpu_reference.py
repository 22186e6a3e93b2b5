"""Reference (CPU, torch fp32) implementations of every EM op.

These are the golden-path semantics the HIP kernels are tested against and
the compute path for CPU-only runs (BASELINE config 1). Shapes follow the
MI355X-native layout:

 - data is dimension-major: ``x`` is [D, N] (gaussian.cu:212-218 transpose,
   kept resident in this layout from the start)
 - memberships / log-weights are cluster-major: ``w`` is [K, N]
   (gaussian.h:75, memberships[c*num_events+e])
 - sufficient statistics: N [K], mean numerators [K, D], second moments
   S [K, D, D] with S_c = sum_e w_ce * x_e x_e^T.

The covariance is finalized as R_c = (S_c - N_c mu_c mu_c^T + reg) / N_c,
algebraically identical to the reference's per-event centered sum
(gaussian_kernel.cu:644-646) because mu_c is the exact weighted mean.
"""
from __future__ import annotations

import math

import torch


LOG_2PI = math.log(2.0 * math.pi)


def estep_logw(x: torch.Tensor, means: torch.Tensor, rinv: torch.Tensor,
               constant: torch.Tensor, pi: torch.Tensor,
               diag_only: bool = False) -> torch.Tensor:
    """Log weighted likelihoods (estep1, gaussian_kernel.cu:383-444).

    x [D, N]; means [K, D]; rinv [K, D, D]; constant [K]; pi [K].
    Returns logw [K, N] = -0.5 * (x-mu)^T Rinv (x-mu) + constant + ln(pi).
    """
    d, n = x.shape
    k = means.shape[0]
    logw = torch.empty((k, n), dtype=torch.float32, device=x.device)
    for c in range(k):
        xc = x - means[c].unsqueeze(1)  # [D, N]
        if diag_only:
            q = (xc * xc * torch.diagonal(rinv[c]).unsqueeze(1)).sum(dim=0)
        else:
            q = (xc * (rinv[c] @ xc)).sum(dim=0)
        logw[c] = -0.5 * q + constant[c] + torch.log(pi[c])
    return logw


def estep_posteriors(logw: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Posteriors + total log-likelihood (estep2, gaussian_kernel.cu:446-512).

    Returns (w [K, N] with columns summing to 1, likelihood scalar tensor).
    Log-sum-exp with per-event max for stability, like the reference.
    """
    denom = estep_lse(logw)
    w = torch.exp(logw - denom.unsqueeze(0))
    return w, denom.sum()


def estep_lse(logw: torch.Tensor) -> torch.Tensor:
    """Per-event log-sum-exp [N] of logw [K, N]: ln p(x_e)."""
    m = logw.max(dim=0).values  # [N]
    return m + torch.log(torch.exp(logw - m.unsqueeze(0)).sum(dim=0))


def event_weight_lse(lse: torch.Tensor, s: torch.Tensor, lns: torch.Tensor
                     ) -> tuple[torch.Tensor, torch.Tensor]:
    """CPU twin of the event-weight kernel: (lse_w [N], weighted likelihood).

    lse_w = lse - lns with +inf where s == 0 (lns = ln s, -inf there), so
    exp(logw - lse_w) = s * posterior with an exact 0 at zero weights. The
    likelihood is sum_e s_e lse_e over the events with s_e > 0 (0 * inf is
    NaN, so zero-weight terms are skipped, not multiplied)."""
    zero = s == 0
    inf = torch.full_like(lse, float("inf"))
    lse_w = torch.where(zero, inf, lse - lns)
    lik = torch.where(zero, torch.zeros_like(lse), s * lse).sum()
    return lse_w, lik


def estep_posteriors_weighted(logw: torch.Tensor, s: torch.Tensor
                              ) -> tuple[torch.Tensor, torch.Tensor,
                                         torch.Tensor]:
    """E-step of a fit with per-event weights s [N] >= 0: (w [K, N]
    normalized posteriors, w_s [K, N] = w * s — what the M-step sums, its
    columns sum to s — and the likelihood sum_e s_e ln p(x_e))."""
    lse = estep_lse(logw)
    _, lik = event_weight_lse(lse, s, torch.log(s))
    w = torch.exp(logw - lse.unsqueeze(0))
    # a zero-weight event contributes an exact 0 even where its posterior
    # is NaN (lse = -inf)
    w_s = torch.where((s == 0).unsqueeze(0), torch.zeros_like(w),
                      w * s.unsqueeze(0))
    return w, w_s, lik


def background_lse(lse: torch.Tensor, b: float,
                   s: torch.Tensor | None = None
                   ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                              torch.Tensor]:
    """CPU twin of the background kernel for the mixture
    (1 - pi0) sum_c pi_c N_c + pi0 / V with b = ln(pi0 / (1 - pi0)) - ln V:
    (lse_b, lse_m, n0, lik), fp32.

    lse_b = logaddexp(lse, b) (b = -inf: lse itself; both -inf: -inf);
    lse_m is what the M-step subtracts: lse_b, or with weights s
    event_weight_lse of lse_b (lse_b - ln s, +inf at s == 0);
    n0 = sum_e s_e r0_e with r0 = exp(b - lse_b) the background posterior
    and lik = sum_e s_e lse_b_e, zero-weight events skipped."""
    b = float(b)
    if b == float("-inf"):
        lse_b = lse.clone()
        r0 = torch.zeros_like(lse)
    else:
        bt = torch.full_like(lse, b)
        hi = torch.maximum(lse, bt)
        lse_b = hi + torch.log1p(torch.exp(-(lse - bt).abs()))
        r0 = torch.exp(bt - lse_b)
    if s is None:
        return lse_b, lse_b, r0.sum(), lse_b.sum()
    lse_m, lik = event_weight_lse(lse_b, s, torch.log(s))
    n0 = torch.where(s == 0, torch.zeros_like(r0), s * r0).sum()
    return lse_b, lse_m, n0, lik


def background_update(n0: float, n_total: float, log_volume: float
                      ) -> tuple[float, float, float]:
    """(pi0, b, lik_add) of the background after an E-step that gave the
    background n0 of n_total observations: pi0 = min(n0 / n_total,
    1 - 1e-6), b = ln pi0 - ln(1 - pi0) - ln V (-inf at pi0 == 0) and
    lik_add = n_total ln(1 - pi0), the term that completes
    ln L = sum lse_b + lik_add. Float64 scalars (the kernel's own tail)."""
    pi0 = float(n0) / float(n_total)
    if not pi0 > 0.0:
        pi0 = 0.0
    pi0 = min(pi0, 1.0 - 1e-6)
    l1m = math.log1p(-pi0)
    b = (math.log(pi0) - l1m - float(log_volume)) if pi0 > 0.0 \
        else float("-inf")
    return pi0, b, float(n_total) * l1m


def estep_posteriors_background(logw: torch.Tensor, b: float,
                                s: torch.Tensor | None = None
                                ) -> tuple[torch.Tensor, torch.Tensor | None,
                                           torch.Tensor, torch.Tensor,
                                           torch.Tensor]:
    """E-step of a fit with a background: (w [K, N] = exp(logw - lse_b), the
    Gaussian posteriors — their columns sum to 1 - r0 —, w_s = w * s for
    the M-step of a weighted fit (else None), lse_b [N], n0, lik)."""
    lse = estep_lse(logw)
    lse_b, _, n0, lik = background_lse(lse, b, s)
    w = torch.exp(logw - lse_b.unsqueeze(0))
    w_s = None
    if s is not None:
        w_s = torch.where((s == 0).unsqueeze(0), torch.zeros_like(w),
                          w * s.unsqueeze(0))
    return w, w_s, lse_b, n0, lik


def student_t_delta(nu: float, d: int) -> float:
    """delta(nu, D) = lgamma((nu + D) / 2) - lgamma(nu / 2) - D/2 ln(nu / 2):
    what the t normaliser adds to the Gaussian ``constant`` (float64; the
    same for every cluster). It tends to 0 as nu grows."""
    nu = float(nu)
    return (math.lgamma(0.5 * (nu + d)) - math.lgamma(0.5 * nu)
            - 0.5 * d * math.log(0.5 * nu))


def student_t_lse(logw: torch.Tensor, add: torch.Tensor, nu: float, d: int,
                  s: torch.Tensor | None = None, train: bool = True
                  ) -> tuple[torch.Tensor, torch.Tensor,
                             torch.Tensor | None, torch.Tensor | None,
                             torch.Tensor | None]:
    """CPU twin of the Student-t kernel, fp32: Gaussian log-weights
    logw [K, N] = add_c - q/2 become t ones.

    q = max(0, 2 (add_c - logw)); lt = add_c + delta - (nu + D)/2 log1p(q/nu);
    lse_t = logsumexp_c lt (-inf where every lt is); u = (nu + D)/(nu + q).
    Returns (logw_out, lse_t, lse_m, n_c, lik). ``train``: logw_out =
    lt + ln u, lse_m = lse_t or event_weight_lse of it with weights s,
    n_c [K] = sum_e s_e exp(lt - lse_t) and lik = sum_e s_e lse_t, zero-weight
    events skipped and events with lse_t = -inf adding exact zeros to n_c.
    Posterior mode: logw_out = lt and the last three are None."""
    lt, lnu, lse_t, dead = _student_t_terms(logw, add, nu, d)
    if not train:
        return lt, lse_t, None, None, None
    out = lt + lnu
    tau = _student_t_tau(lt, lse_t, dead)
    if s is None:
        return out, lse_t, lse_t, tau.sum(dim=1), lse_t.sum()
    lse_m, lik = event_weight_lse(lse_t, s, torch.log(s))
    n_c = torch.where((s == 0).unsqueeze(0), torch.zeros_like(tau),
                      tau * s.unsqueeze(0)).sum(dim=1)
    return out, lse_t, lse_m, n_c, lik


def _student_t_terms(logw: torch.Tensor, add: torch.Tensor, nu: float,
                     d: int) -> tuple[torch.Tensor, torch.Tensor,
                                      torch.Tensor, torch.Tensor]:
    """(lt [K, N], ln u [K, N], lse_t [N], dead [N]: every lt is -inf)."""
    nu32 = torch.tensor(float(nu), dtype=torch.float32)
    nud = torch.tensor(float(nu) + float(d), dtype=torch.float32)
    delta = torch.tensor(student_t_delta(nu, d), dtype=torch.float32)
    a = add.unsqueeze(1)
    q = (2.0 * (a - logw)).clamp(min=0.0)
    lt = (a + delta) - (0.5 * nud) * torch.log1p(q / nu32)
    m = lt.max(dim=0).values
    dead = m == float("-inf")
    m_safe = torch.where(dead, torch.zeros_like(m), m)
    lse_t = torch.where(
        dead, m, m_safe + torch.log(torch.exp(lt - m_safe.unsqueeze(0))
                                    .sum(dim=0)))
    return lt, torch.log(nud / (nu32 + q)), lse_t, dead


def _student_t_tau(lt: torch.Tensor, lse_t: torch.Tensor,
                   dead: torch.Tensor) -> torch.Tensor:
    """exp(lt - lse_t), exact zeros for the events whose lt are all -inf."""
    safe = torch.where(dead, torch.zeros_like(lse_t), lse_t)
    return torch.where(dead.unsqueeze(0), torch.zeros_like(lt),
                       torch.exp(lt - safe.unsqueeze(0)))


def student_t_pi(n_c: torch.Tensor, constant: torch.Tensor | None = None
                 ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor | None]:
    """CPU twin of the one-block kernel after finalize: (N, pi, add) of a t
    fit from the reduced responsibilities n_c [K] = sum_e s_e tau_ce.
    pi = n_c / sum n_c (summed in cluster order in fp32), 1e-10 where
    n_c < 0.5; add = constant + ln pi when ``constant`` is given."""
    total = torch.zeros((), dtype=torch.float32)
    for c in range(int(n_c.numel())):
        total = total + n_c[c]
    pi = torch.where(n_c < 0.5, torch.full_like(n_c, 1e-10), n_c / total)
    add = None if constant is None else constant + torch.log(pi)
    return n_c.clone(), pi, add


def estep_posteriors_student_t(logw: torch.Tensor, add: torch.Tensor,
                               nu: float, d: int,
                               s: torch.Tensor | None = None
                               ) -> tuple[torch.Tensor, torch.Tensor,
                                          torch.Tensor, torch.Tensor]:
    """E-step of a t fit on the CPU engine: (tau [K, N], the t posteriors;
    w_m = s tau u, what the parameter-expanded M-step sums; n_c [K];
    lik)."""
    lt, lnu, lse_t, dead = _student_t_terms(logw, add, nu, d)
    # the kernel's arithmetic: tau = exp(lt - lse_t) for output, and the
    # M-step weight exp((lt + ln u) - lse_m) with lse_m = lse_t - ln s
    tau = torch.exp(lt - lse_t.unsqueeze(0))
    tau_n = _student_t_tau(lt, lse_t, dead)
    if s is None:
        lse_m, lik, n_c = lse_t, lse_t.sum(), tau_n.sum(dim=1)
    else:
        lse_m, lik = event_weight_lse(lse_t, s, torch.log(s))
        n_c = torch.where((s == 0).unsqueeze(0), torch.zeros_like(tau_n),
                          tau_n * s.unsqueeze(0)).sum(dim=1)
    w_m = torch.exp((lt + lnu) - lse_m.unsqueeze(0))
    # exact zeros only where the contract has them: events with s == 0 and
    # events whose lt are all -inf; any other NaN stays visible
    zero = dead if s is None else dead | (s == 0)
    w_m = torch.where(zero.unsqueeze(0), torch.zeros_like(w_m), w_m)
    return tau, w_m, n_c, lik


def student_t_posteriors(logw: torch.Tensor, add: torch.Tensor, nu: float,
                         d: int) -> tuple[torch.Tensor, torch.Tensor,
                                          torch.Tensor]:
    """(lt [K, N], lse_t [N], tau [K, N] = exp(lt - lse_t)) from Gaussian
    log-weights: the output and scoring path (posterior mode)."""
    lt, lse_t, _, _, _ = student_t_lse(logw, add, nu, d, None, False)
    return lt, lse_t, torch.exp(lt - lse_t.unsqueeze(0))


def classify(x: torch.Tensor, means: torch.Tensor, rinv: torch.Tensor,
             constant: torch.Tensor, pi: torch.Tensor,
             diag_only: bool = False
             ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Score events x [D, N] against a mixture: (label int32 [N], lse [N] =
    ln p(x_e), pmax [N] = posterior of the assigned cluster). The label is
    the first maximum of the posteriors estep_posteriors gives, so it is
    the argmax of a .results row."""
    k = means.shape[0]
    logw = estep_logw(x, means, rinv, constant, pi, diag_only)
    lse = estep_lse(logw)
    w, _ = estep_posteriors(logw)
    pmax = w.max(dim=0).values
    idx = torch.arange(k, dtype=torch.int32).unsqueeze(1)
    first = torch.where(w == pmax.unsqueeze(0), idx,
                        torch.full_like(idx, k)).min(dim=0).values
    # an event whose posteriors are all NaN matches nowhere: keep it in range
    return first.clamp(max=k - 1), lse, pmax


def mstep_sufficient_stats(
    x: torch.Tensor, w: torch.Tensor
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-shard sufficient statistics (mstep_N / mstep_means /
    mstep_covariance1 numerators, gaussian_kernel.cu:522-677).

    Returns (N [K], mean numerators [K, D], S [K, D, D]).
    S is the *uncentered* weighted second moment; centering happens in
    finalize (translation by the global mean is handled by the engine).
    """
    n_c = w.sum(dim=1)                                 # [K]
    mean_num = w @ x.T                                  # [K, D]
    # S_c = (x * w_c) @ x^T, batched over clusters
    k, n = w.shape
    d = x.shape[0]
    s = torch.empty((k, d, d), dtype=x.dtype, device=x.device)
    for c in range(k):
        xw = x * w[c].unsqueeze(0)
        s[c] = xw @ x.T
    return n_c, mean_num, s


def finalize_means(n_c: torch.Tensor, mean_num: torch.Tensor) -> torch.Tensor:
    """means = mean_num / N where N > 0.5 else 0 (gaussian.cu:610-622)."""
    safe = n_c > 0.5
    means = torch.where(
        safe.unsqueeze(1), mean_num / n_c.clamp(min=1e-30).unsqueeze(1),
        torch.zeros_like(mean_num),
    )
    return means


def finalize_covariance(
    n_c: torch.Tensor, means: torch.Tensor, s: torch.Tensor,
    avgvar: torch.Tensor, world_size: int = 1, diag_only: bool = False,
) -> torch.Tensor:
    """Covariance finalize, reproducing the reference exactly.

    Per reference semantics with G total GPUs:
     - each GPU's kernel writes its partial centered sum if global N >= 1.0
       else 0 (gaussian_kernel.cu:658-667), then adds avgvar to the diagonal
       (gaussian_kernel.cu:673-675);
     - the global reduction sums G partials => diagonal receives G*avgvar;
     - the host divides by global N when N > 0.5, else resets to identity
       (gaussian.cu:663-679).

    Here: cov_num = S - N mu mu^T when N >= 1.0 else 0; diagonal += G*avgvar;
    R = cov_num / N when N > 0.5 else I.
    """
    k, d, _ = s.shape
    mu_outer = means.unsqueeze(2) * means.unsqueeze(1)      # [K, D, D]
    cov_num = s - n_c.view(k, 1, 1) * mu_outer
    cov_num = torch.where(
        (n_c >= 1.0).view(k, 1, 1), cov_num, torch.zeros_like(cov_num)
    )
    if diag_only:
        cov_num = torch.diag_embed(torch.diagonal(cov_num, dim1=1, dim2=2))
    eye = torch.eye(d, dtype=s.dtype, device=s.device)
    cov_num = cov_num + (world_size * avgvar).view(k, 1, 1) * eye
    r = torch.where(
        (n_c > 0.5).view(k, 1, 1),
        cov_num / n_c.clamp(min=1e-30).view(k, 1, 1),
        eye.expand(k, d, d),
    )
    return r.contiguous()


def lu_invert_nopivot(a: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Batched no-pivot LU inversion + ln|det| on fp32 tensors.

    Same elimination as the device `invert` (gaussian_kernel.cu:107-169):
    Doolittle LU without pivoting, ln determinant from |diag|, triangular
    inversion, composition. a: [K, D, D]. Returns (inv [K, D, D], logdet [K]).
    """
    k, d, _ = a.shape
    data = a.clone()
    if d == 1:
        logdet = torch.log(data[:, 0, 0])
        return (1.0 / data).reshape(k, 1, 1), logdet
    data[:, 0, 1:] /= data[:, 0, 0].unsqueeze(1)
    for i in range(1, d):
        data[:, i:, i] -= torch.einsum("kjp,kp->kj", data[:, i:, :i], data[:, :i, i])
        if i == d - 1:
            continue
        data[:, i, i + 1:] = (
            data[:, i, i + 1:]
            - torch.einsum("kp,kpj->kj", data[:, i, :i], data[:, :i, i + 1:])
        ) / data[:, i, i].unsqueeze(1)
    diag = torch.diagonal(data, dim1=1, dim2=2).abs()
    logdet = torch.log(diag).sum(dim=1)
    # invert L (Crout storage: L holds the diagonal, U is unit-diagonal)
    for i in range(d):
        for j in range(i, d):
            if i == j:
                x = torch.ones(k, dtype=a.dtype, device=a.device)
            else:
                x = -torch.einsum("kp,kp->k", data[:, j, i:j], data[:, i:j, i])
            data[:, j, i] = x / data[:, j, j]
    # invert U (unit diagonal)
    for i in range(d):
        for j in range(i + 1, d):
            ks = torch.arange(i, j, device=a.device)
            lhs = data[:, ks, j]
            rhs = torch.where(
                (ks == i).unsqueeze(0), torch.ones_like(lhs), data[:, i, ks]
            )
            data[:, i, j] = -(lhs * rhs).sum(dim=1)
    # final composition out[j,i] = sum_k Uinv[j,k>=] * Linv[k,i]
    out = torch.empty_like(data)
    for i in range(d):
        for j in range(d):
            k0 = max(i, j)
            ks = torch.arange(k0, d, device=a.device)
            lhs = torch.where(
                (ks == j).unsqueeze(0),
                torch.ones(1, len(ks), dtype=a.dtype, device=a.device),
                data[:, j, ks],
            )
            out[:, j, i] = (lhs * data[:, ks, i]).sum(dim=1)
    return out, logdet


def lu_logdet_nopivot(a: torch.Tensor) -> torch.Tensor:
    """Batched ln|det| via the same no-pivot elimination as
    lu_invert_nopivot, without the inversion phases. a: [K, D, D]."""
    k, d, _ = a.shape
    data = a.clone()
    if d == 1:
        return torch.log(data[:, 0, 0].abs())
    data[:, 0, 1:] /= data[:, 0, 0].unsqueeze(1)
    for i in range(1, d):
        data[:, i:, i] -= torch.einsum("kjp,kp->kj", data[:, i:, :i], data[:, :i, i])
        if i == d - 1:
            continue
        data[:, i, i + 1:] = (
            data[:, i, i + 1:]
            - torch.einsum("kp,kpj->kj", data[:, i, :i], data[:, :i, i + 1:])
        ) / data[:, i, i].unsqueeze(1)
    diag = torch.diagonal(data, dim1=1, dim2=2).abs()
    return torch.log(diag).sum(dim=1)


def compute_constants(r: torch.Tensor,
                      diag_only: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """Rinv + per-cluster constant (constants_kernel, gaussian_kernel.cu:196-243).

    constant = -D/2*ln(2*pi) - 0.5*ln|R| (natural log on the GPU path).
    """
    k, d, _ = r.shape
    if diag_only:
        diag = torch.diagonal(r, dim1=1, dim2=2)
        logdet = torch.log(diag.prod(dim=1))
        rinv = torch.diag_embed(1.0 / diag)
    else:
        rinv, logdet = lu_invert_nopivot(r)
    constant = -d * 0.5 * LOG_2PI - 0.5 * logdet
    return rinv, constant


def compute_pi(n_c: torch.Tensor) -> torch.Tensor:
    """pi = N / sum(N), floored at 1e-10 for N < 0.5
    (compute_pi, gaussian_kernel.cu:172-193, with the K>256 indexing bug
    fixed — SURVEY §2.6 #3)."""
    total = n_c.sum()
    pi = n_c / total
    return torch.where(n_c < 0.5, torch.full_like(pi, 1e-10), pi)
